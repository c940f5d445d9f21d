"""GPU suite: the one form of a staged host-pointer call (pcx_host.hpp host_call) under every handle that goes through it.

The same input is handed to a handle three ways -- as a pageable numpy array (staged in pieces through the handle's workspaces), in
page-locked slabs (the kernels address the caller's memory in place) and as device memory through process_dev -- and once mixed,
pageable in and page-locked out.  All four must return the same bytes, and leave the same carried state where the handle has a
getter for it.  Every handle is called twice, so that the second call of a stateful one starts from what the first left.

Sizes are the smallest that reach each branch of the staging: one element, an odd count of a few thousand, and a count whose larger
direction is just over 1 MiB + 4 KiB (stage_piece cuts at 1 MiB: two pieces, the last one ragged).

Then the overlap rule of in and out (pcx_host.hpp buffers_ok) on device pointers, handle by handle."""
import ctypes as C

import numpy as np
import pytest

from pothoscomms_amd import _lib, device
from tests.util import Pinned

pytestmark = pytest.mark.gpu

PIECE = (1 << 20) + 4096
QPSK = np.array([[-1, -1], [-1, 1], [1, 1], [1, -1]], np.float64)
PREAMBLE = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1], np.uint8)
FM_TAPS = 31


class Case:
    """one handle: how to make it, its input for n units of work, the bytes in and out, and its three entry points"""

    def __init__(self, make, data, in_bytes, out_bytes, host, dev, state=None, unit=lambda h: 1):
        self.make, self.data, self.in_bytes, self.out_bytes, self.host, self.dev, self.state, self.unit = (
            make, data, in_bytes, out_bytes, host, dev, state, unit)


def _simple(name):
    """entry points of the shape (h, in, out, n) and (h, in, out, n, stream)"""
    L = _lib.load()
    return (lambda h, x, y, n: _lib.check(getattr(L, name + "_process")(h._h, x, y, n)),
            lambda h, x, y, n: _lib.check(getattr(L, name + "_process_dev")(h._h, x, y, n, device._stream_ptr())))


def _uniform(dtype, width):
    return lambda rng, n: rng.uniform(-1, 1, (n, width) if width > 1 else (n,)).astype(dtype)


def _bytes_below(top):
    return lambda rng, n: rng.integers(0, top, n, dtype=np.uint8)


def _fm_host(h, x, y, n):
    c, p = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.load().pcx_fmchain_process(h._h, x, n + FM_TAPS - 1, y, n, C.byref(c), C.byref(p)))
    assert (c.value, p.value) == (n, n)


def _fm_dev(h, x, y, n):
    c, p = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.load().pcx_fmchain_process_dev(h._h, x, n + FM_TAPS - 1, y, n, C.byref(c), C.byref(p), device._stream_ptr()))
    assert (c.value, p.value) == (n, n)


def _fm_chain():
    ch = device.FmChain()
    ch.set_phase(0.7)
    ch.set_taps(np.hanning(FM_TAPS + 2)[1:-1] / 16, False)
    return ch


def _distances_host(h, x, y, n):
    npos = C.c_size_t()
    _lib.check(_lib.load().pcx_preamble_distances(h._h, x, n + PREAMBLE.size, y, C.byref(npos)))
    assert npos.value == n


def _cases():
    L = _lib.load()
    P = PREAMBLE.size
    return {
        "dcremoval": Case(lambda: device.DCRemoval("complex_float32", 16, 2), _uniform(np.float32, 2),
                          lambda n: 8 * n, lambda n: 8 * n, *_simple("pcx_dcremoval")),
        # a lookahead: n + 3 elements in for n floats out
        "envelope": Case(lambda: device.EnvelopeDetector("complex_float32", attack=5, release=50, lookahead=3),
                         lambda rng, n: _uniform(np.float32, 2)(rng, n + 3), lambda n: 8 * (n + 3), lambda n: 4 * n,
                         *_simple("pcx_envelope"), state=lambda h: np.float32(h.state()).tobytes()),
        "iir": Case(lambda: device.IIRFilter("float32"), _uniform(np.float32, 1), lambda n: 4 * n, lambda n: 4 * n, *_simple("pcx_iir")),
        "scrambler": Case(lambda: device.Scrambler(False, "multiplicative", 0x11021, 0xACE1), _bytes_below(256),
                          lambda n: n, lambda n: n, *_simple("pcx_scrambler"), state=lambda h: h.state()),
        # complex_float64: one byte against sixteen
        "mapper": Case(lambda: device.SymbolMapper("complex_float64", QPSK), _bytes_below(256),
                       lambda n: n, lambda n: 16 * n, *_simple("pcx_mapper")),
        "slicer": Case(lambda: device.SymbolSlicer("complex_float64", QPSK), _uniform(np.float64, 2),
                       lambda n: 16 * n, lambda n: n, *_simple("pcx_slicer")),
        "diffcode": Case(lambda: device.DifferentialCoder(False, 4), _bytes_below(4),
                         lambda n: n, lambda n: n, *_simple("pcx_diffcode"), state=lambda h: h.state()),
        # three payload bytes become eight 3-bit symbols: whole groups only
        "repack": Case(lambda: device.SymbolRepacker("bytes_to_symbols", 3, "MSBit"), _bytes_below(256),
                       lambda n: n, lambda n: n // 3 * 8, *_simple("pcx_repack"), unit=lambda h: h.group()[0]),
        "preamble_distances": Case(lambda: device.PreambleCorrelator(PREAMBLE, threshold=2), lambda rng, n: _bytes_below(2)(rng, n + P),
                                   lambda n: n + P, lambda n: 4 * n, _distances_host,
                                   lambda h, x, y, n: _lib.check(L.pcx_preamble_distances_dev(h._h, x, n + P, y, device._stream_ptr()))),
        # n frames of 16 bins
        "fft": Case(lambda: device.Fft("complex_float32", 16, False), lambda rng, n: _uniform(np.float32, 2)(rng, 16 * n),
                    lambda n: 128 * n, lambda n: 128 * n,
                    lambda h, x, y, n: _lib.check(L.pcx_fft_transform(h._h, x, y, n)),
                    lambda h, x, y, n: _lib.check(L.pcx_fft_transform_dev(h._h, x, y, n, device._stream_ptr()))),
        "freqdemod": Case(lambda: device.FreqDemod("complex_float32"), _uniform(np.float32, 2),
                          lambda n: 8 * n, lambda n: 4 * n, *_simple("pcx_freqdemod")),
        "fmchain": Case(_fm_chain, lambda rng, n: _uniform(np.float32, 2)(rng, n + FM_TAPS - 1),
                        lambda n: 8 * (n + FM_TAPS - 1), lambda n: 4 * n, _fm_host, _fm_dev),
    }


NAMES = ["dcremoval", "envelope", "iir", "scrambler", "mapper", "slicer", "diffcode", "repack", "preamble_distances", "fft", "freqdemod",
         "fmchain"]


def _two_calls(case, call):
    """a fresh handle called twice on the same input: (bytes of the first call, bytes of the second, carried state)"""
    h = case.make()
    try:
        a = call(h)
        b = call(h)
        return a, b, case.state(h) if case.state else None
    finally:
        h.close()


@pytest.mark.parametrize("size", ["one", "odd", "two_pieces"])
@pytest.mark.parametrize("name", NAMES)
def test_host_and_device_calls_return_the_same_bytes(name, size):
    import torch
    case = _cases()[name]
    h = case.make()
    unit = case.unit(h)
    h.close()
    larger = lambda n: max(case.in_bytes(n), case.out_bytes(n))      # noqa: E731
    if size == "two_pieces":
        # the first whole unit at which the larger direction passes 1 MiB + 4 KiB
        n = (PIECE * 1024 // (larger(2048 * unit) - larger(1024 * unit)) - 64) * unit
        while larger(n) <= PIECE:
            n += unit
        assert PIECE < larger(n) <= PIECE + 128
    else:
        n = -(-{"one": 1, "odd": 4099}[size] // unit) * unit
    nin, nout = case.in_bytes(n), case.out_bytes(n)
    x = np.ascontiguousarray(case.data(np.random.default_rng(n), n)).view(np.uint8).reshape(-1)
    assert x.size == nin

    # device memory through process_dev: the reference of the other three
    xd = torch.from_numpy(x).cuda()

    def on_device(h):
        yd = torch.full((nout,), 0xAA, dtype=torch.uint8, device="cuda")
        case.dev(h, C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), n)
        torch.cuda.synchronize()
        return yd.cpu().numpy().tobytes()
    want = _two_calls(case, on_device)
    assert case.state is None or want[2] is not None

    def pageable(h):
        y = np.full(nout, 0xAA, np.uint8)
        case.host(h, x.ctypes.data, y.ctypes.data, n)
        return y.tobytes()
    got = _two_calls(case, pageable)
    assert got == want, "pageable"

    pin, pout = Pinned((nin,), np.uint8), Pinned((nout,), np.uint8)
    try:
        pin.a[:] = x

        def into_slab(src):
            def call(h):
                pout.a[:] = 0xAA
                case.host(h, src, pout.a.ctypes.data, n)
                return pout.a.tobytes()
            return call
        got = _two_calls(case, into_slab(pin.a.ctypes.data))
        assert got == want, "page-locked"
        got = _two_calls(case, into_slab(x.ctypes.data))
        assert got == want, "pageable in, page-locked out"
    finally:
        pin.free(); pout.free()


# handle, bytes of one input element, input elements of the call, bytes in, bytes out, out == in accepted, the refusal's text
OVERLAP = [
    ("scrambler", 1, 1024, 1024, 1024, True, "scrambler: out overlaps in (in place means out == in)"),
    ("diffcode", 1, 1024, 1024, 1024, True, "differential coder: out overlaps in (in place means out == in)"),
    ("preamble", 1, 1024, 1024, 1024 - 16, True, "preamble correlator: out overlaps in (in place means out == in)"),
    ("iir", 4, 1024, 4096, 4096, False, "iir_filter: out overlaps in (out == in included)"),
    ("mapper", 1, 1024, 1024, 16384, False, "symbol mapper: out overlaps in"),
    ("slicer", 16, 1024, 16384, 1024, False, "symbol slicer: out overlaps in"),
    ("repack", 1, 3072, 3072, 8192, False, "bytes to symbols: out overlaps in"),
]


@pytest.mark.parametrize("name,elem,n,nin,nout,in_place,text", OVERLAP, ids=[row[0] for row in OVERLAP])
def test_overlap_contract_on_device_pointers(name, elem, n, nin, nout, in_place, text):
    """out == in is in place where the element sizes agree and the kernels allow it, refused elsewhere; out one element into in is
    refused everywhere; out directly behind in is accepted everywhere.  A refusal comes back before anything is launched."""
    import torch
    L = _lib.load()
    cases = _cases()
    h = cases["preamble_distances" if name == "preamble" else name].make()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    base = buf.data_ptr()
    assert nin + max(nin, nout) <= buf.numel()

    def call(out_off):
        i, o, st = C.c_void_p(base), C.c_void_p(base + out_off), device._stream_ptr()
        if name == "preamble":
            return L.pcx_preamble_process_dev(h._h, i, n, o, None, 0, C.c_void_p(counts.data_ptr()), C.c_void_p(counts.data_ptr() + 8), st)
        return getattr(L, "pcx_" + name + "_process_dev")(h._h, i, o, n, st)
    try:
        if in_place:
            assert call(0) == _lib.OK, _lib.last_error()
        else:
            assert call(0) == _lib.ERR_ARG and _lib.last_error() == text
        assert call(elem) == _lib.ERR_ARG and _lib.last_error() == text
        assert call(nin) == _lib.OK, _lib.last_error()
        torch.cuda.synchronize()
    finally:
        h.close()
