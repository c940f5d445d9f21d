"""Every plan of pcx_fir_process_dev through one table.

fir_process_dev_impl (pothoscomms_amd/csrc/pcx_fir_api.hip) picks one of about twenty plans from the handle's tables, and the
AUTO choice above it picks the algorithm.  PLANS below holds at least one row for each branch of both, and a row on either side
of every bound that decides a plan.  Each row names the last_algo the call must report.  Three checks run over the table:

1. guard bands and misaligned windows: input and output windows at element offsets 0, 1 and 3 inside poisoned buffers (NaN for
   floats, the type's extreme values for integers).  The outputs equal the oracle's work() on the window (bit for bit for integer
   and EXACT plans, otherwise within the bar of that plan's own parity test), no poison is written or read, and the three offsets
   give the same bits.  (Offsets count whole elements: a 16-byte element, complex float64 or complex int64, stays 16-byte aligned.)
2. reconfiguration: one handle per stream type walks through that type's rows, shuffled, three times, with the setters alone.
   Every call equals, bit for bit, a fresh handle given the same settings: no table of an earlier plan leaks into the next.
3. the gated call: only complex_float32 with M = L = 1, K <= 2049 on the overlap-save plan has a gate (include/pcx.h).  That
   plan must run gated and equal the plain call; every other row must return gated = 0 with nothing queued or written.
"""
import collections
import zlib

import numpy as np
import pytest

from tests.util import TOL, bands_intact, diff_note, guarded, h2d

pytestmark = pytest.mark.gpu

Row = collections.namedtuple("Row", "name dtype taps ntaps L M algo want bar tapgen")


def R(name, dtype, taps, ntaps, L=1, M=1, algo="AUTO", want="OLS_FFT", bar=None, tapgen="normal"):
    return Row(name, dtype, taps, ntaps, L, M, algo, want, bar, tapgen)


# bar: None = the default of the type (integers and EXACT bit for bit, float64 1e-13, float32 TOL); a number = the float32 bar of
# that plan's own parity test (tests/test_parity_gpu.py, tests/test_fuzz_gpu.py)
PLANS = [
    # -- complex_float32, M = L = 1 (fir_fast_applicable) --
    R("cf32 direct tile K=1 (AUTO: the unit tap stays exact)", "complex_float32", "COMPLEX", 1, want="DIRECT"),
    R("cf32 direct tile K=255 DIRECT", "complex_float32", "COMPLEX", 255, algo="DIRECT", want="DIRECT"),
    R("cf32 4096-sample K=1 OLS_FFT", "complex_float32", "COMPLEX", 1, algo="OLS_FFT"),
    R("cf32 4096-sample K=255", "complex_float32", "COMPLEX", 255),
    R("cf32 4096-sample K=2049 real taps", "complex_float32", "REAL", 2049),
    R("cf32 4096-sample K=2049", "complex_float32", "COMPLEX", 2049),
    R("cf32 partitioned K=2050", "complex_float32", "COMPLEX", 2050),
    R("cf32 partitioned K=4097", "complex_float32", "COMPLEX", 4097),
    R("cf32 partitioned K=8193", "complex_float32", "COMPLEX", 8193),
    R("cf32 sliding EXACT K=8194 (beyond every frequency-domain plan)", "complex_float32", "COMPLEX", 8194, want="EXACT"),
    # -- complex_float32 decimating: the folded spectrum (have_decim) for M = 2 and 4 / 8 / 16-fold, the strided polyphase kernel else --
    R("cf32 decim M=2", "complex_float32", "COMPLEX", 63, M=2),
    R("cf32 decim M=4", "complex_float32", "REAL", 100, M=4),
    R("cf32 decim M=8", "complex_float32", "COMPLEX", 255, M=8),
    R("cf32 decim M=8 K=2049", "complex_float32", "COMPLEX", 2049, M=8),
    R("cf32 decim M=16", "complex_float32", "COMPLEX", 255, M=16),
    R("cf32 decim M=160 (16-fold, one in 10 stored)", "complex_float32", "COMPLEX", 1000, M=160),
    R("cf32 poly strided M=3", "complex_float32", "COMPLEX", 100, M=3),
    R("cf32 poly strided M=6 (2-fold: not folded)", "complex_float32", "REAL", 100, M=6),
    R("cf32 poly strided L=3 M=2", "complex_float32", "COMPLEX", 61, L=3, M=2),
    # -- complex_float32 interpolating: the replicated spectrum (have_interp, L in 2/4/8/16), polyphase rows otherwise --
    R("cf32 interp L=2", "complex_float32", "COMPLEX", 64, L=2),
    R("cf32 interp L=4 K=513 (kov_in = 512, at its bound)", "complex_float32", "COMPLEX", 2049, L=4),
    R("cf32 interp L=8", "complex_float32", "COMPLEX", 200, L=8),
    R("cf32 interp L=16 K=129 (kov_in = 128 at its bound, 2049 taps)", "complex_float32", "REAL", 2049, L=16),
    R("cf32 poly rows L=16 2050 taps (past the replicated plan)", "complex_float32", "REAL", 2050, L=16),
    R("cf32 poly rows L=3 M=1", "complex_float32", "COMPLEX", 150, L=3),
    # -- float32 (and complex_float32) long rows / long decimators: the partitioned kernel --
    R("cf32 upols rows L=2 K=2050", "complex_float32", "COMPLEX", 4100, L=2, bar=2 * TOL),
    R("cf32 upols decim M=3 K=3000", "complex_float32", "COMPLEX", 3000, M=3, bar=2 * TOL),
    R("f32 upols rows L=3 K=2050", "float32", "REAL", 6150, L=3, bar=2 * TOL),
    R("f32 upols decim M=2 K=16", "float32", "REAL", 16, M=2, bar=2 * TOL),
    R("f32 generic M=2 K=15 (below the decimating plan)", "float32", "REAL", 15, M=2, want="DIRECT"),
    # -- float32, M = L = 1: two real blocks per transform, beyond 2049 taps the halves side by side --
    R("f32 sliding K=1", "float32", "REAL", 1, want="DIRECT"),
    R("f32 real ols K=2049", "float32", "REAL", 2049),
    R("f32 real ols partitioned K=2050", "float32", "REAL", 2050, bar=3 * TOL),
    # -- float32 interpolating rows on the float kernel (have_interp_f32, 16 <= K <= 2049 under AUTO) --
    R("f32 generic L=3 K=15 (below the interpolating rows)", "float32", "REAL", 45, L=3, want="DIRECT"),
    R("f32 interp rows L=3 K=16", "float32", "REAL", 46, L=3),
    R("f32 interp rows L=5 M=3 K=16", "float32", "REAL", 80, L=5, M=3),
    R("f32 interp rows L=5 M=3 K=2049", "float32", "REAL", 10245, L=5, M=3),
    # -- complex_float64 (have_ols64 from K = 4, M > 1 from 16; have_interp64 to L = 64) --
    R("cf64 sliding K=3", "complex_float64", "COMPLEX", 3, want="DIRECT"),
    R("cf64 ols K=4", "complex_float64", "COMPLEX", 4),
    R("cf64 ols K=2049 (4096 block)", "complex_float64", "REAL", 2049),
    R("cf64 ols K=2050 (8192 block)", "complex_float64", "COMPLEX", 2050),
    R("cf64 ols K=4097", "complex_float64", "COMPLEX", 4097),
    R("cf64 sliding K=4098", "complex_float64", "COMPLEX", 4098, want="DIRECT"),
    R("cf64 generic M=2 K=15", "complex_float64", "COMPLEX", 15, M=2, want="DIRECT"),
    R("cf64 ols decim M=2 K=16", "complex_float64", "COMPLEX", 16, M=2),
    R("cf64 ols decim M=65535", "complex_float64", "COMPLEX", 16, M=65535),
    R("cf64 generic M=65536 (past the decimating plans)", "complex_float64", "COMPLEX", 16, M=65536, want="DIRECT"),
    R("cf64 interp64 L=64", "complex_float64", "COMPLEX", 1280, L=64),
    R("cf64 generic L=65", "complex_float64", "COMPLEX", 1300, L=65, want="DIRECT"),
    # -- complex_int16 (have_ols_int from 64 taps while ||h_q||^2 < 2^44; the packed dot-product kernel below) --
    R("ci16 dot2 K=40", "complex_int16", "COMPLEX", 40, want="EXACT", tapgen="q16"),
    R("ci16 sliding K=63 real taps", "complex_int16", "REAL", 63, want="EXACT"),
    R("ci16 ols K=64", "complex_int16", "COMPLEX", 64),
    R("ci16 ols K=2049", "complex_int16", "COMPLEX", 2049),
    R("ci16 ols K=2050", "complex_int16", "COMPLEX", 2050),
    R("ci16 ols K=4097", "complex_int16", "REAL", 4097),
    R("ci16 dot2 K=4098", "complex_int16", "COMPLEX", 4098, want="EXACT"),
    R("ci16 ols ||h_q||^2 below 2^44", "complex_int16", "COMPLEX", 64, tapgen=5.6 + 5.6j),
    R("ci16 sliding ||h_q||^2 above 2^44", "complex_int16", "COMPLEX", 64, want="EXACT", tapgen=5.7 + 5.7j),
    R("ci16 generic M=2 K=31", "complex_int16", "COMPLEX", 31, M=2, want="EXACT"),
    R("ci16 ols decim M=2 K=32", "complex_int16", "COMPLEX", 32, M=2),
    R("ci16 interp64 L=64", "complex_int16", "COMPLEX", 1280, L=64),
    R("ci16 interp64 L=3 M=2", "complex_int16", "COMPLEX", 60, L=3, M=2),
    # -- complex_int8 (have_ols_int from 96 taps) --
    R("ci8 dot2 K=40", "complex_int8", "COMPLEX", 40, want="EXACT"),
    R("ci8 dot2 K=95", "complex_int8", "COMPLEX", 95, want="EXACT"),
    R("ci8 ols K=96", "complex_int8", "COMPLEX", 96),
    R("ci8 interp64 L=64", "complex_int8", "COMPLEX", 1280, L=64),
    R("ci8 generic L=65", "complex_int8", "COMPLEX", 1300, L=65, want="EXACT"),
    # -- REAL float64 / int16 / int8 on the double pipeline (have_ols_real64 from 24 / 48 taps, M > 1 from 16; have_interp_real) --
    R("f64 sliding K=23", "float64", "REAL", 23, want="DIRECT"),
    R("f64 real ols K=24", "float64", "REAL", 24),
    R("f64 real ols K=4097 (8192 block)", "float64", "REAL", 4097),
    R("f64 sliding K=4098", "float64", "REAL", 4098, want="DIRECT"),
    R("f64 real ols decim M=3 K=16", "float64", "REAL", 16, M=3),
    R("f64 interp real L=3", "float64", "REAL", 120, L=3),
    R("i16 sliding K=47", "int16", "REAL", 47, want="EXACT"),
    R("i16 real ols K=48", "int16", "REAL", 48),
    R("i16 real ols K=2049", "int16", "REAL", 2049),
    R("i16 real ols K=2050", "int16", "REAL", 2050),
    R("i16 real ols K=4097", "int16", "REAL", 4097),
    R("i16 sliding K=4098", "int16", "REAL", 4098, want="EXACT"),
    R("i16 interp real L=4 M=3", "int16", "REAL", 80, L=4, M=3),
    R("i8 sliding K=47", "int8", "REAL", 47, want="EXACT"),
    R("i8 real ols K=48", "int8", "REAL", 48),
    R("i8 interp real L=2", "int8", "REAL", 32, L=2),
    R("i8 generic L=2 K=15", "int8", "REAL", 30, L=2, want="EXACT"),
    # -- the wide integer types: the time-domain kernels only --
    R("ci32 sliding K=3", "complex_int32", "COMPLEX", 3, want="EXACT"),
    R("ci32 generic L=3 M=2", "complex_int32", "COMPLEX", 13, L=3, M=2, want="EXACT"),
    R("i64 sliding K=3", "int64", "REAL", 3, want="EXACT"),
    R("ci64 generic L=2 M=3", "complex_int64", "REAL", 9, L=2, M=3, want="EXACT"),
]
IDS = [r.name for r in PLANS]


def _setup():
    import torch

    from oracle import oracle as o
    return torch, o, {o.F32: torch.float32, o.F64: torch.float64, o.I64: torch.int64, o.I32: torch.int32, o.I16: torch.int16,
                      o.I8: torch.int8}


def _K(row):
    return -(-row.ntaps // row.L)


def _taps(row):
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    n, cplx = row.ntaps, row.taps == "COMPLEX"
    if isinstance(row.tapgen, complex):                            # every tap the same: a chosen ||h_q||
        return np.full(n, row.tapgen) if cplx else np.full(n, row.tapgen.real)
    if row.tapgen == "q16":                                        # Q16.16 images inside +-32767 (the packed kernel's range)
        return rng.uniform(-0.49, 0.49, n) + (1j * rng.uniform(-0.49, 0.49, n) if cplx else 0)
    t = rng.normal(size=n) / np.sqrt(max(1, _K(row)))
    if cplx:
        t = t + 1j * rng.normal(size=n) / np.sqrt(max(1, _K(row)))
    return t * 0.9


def _stream(row, o, scalar, cplx):
    """(input, n_in, n_out): a few 4096-sample blocks of input with ragged ends (a few hundred iterations for 64-fold
    interpolation, three outputs for the largest decimations)"""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()) + 1)
    K = _K(row)
    it = 3 * row.M + 1234 if row.M >= 1000 else 777 + row.M // 2 if row.L >= 32 else 2 * 4096 + 777 + row.M // 2
    n_in = K - 1 + it
    n_out = (it // row.M) * row.L
    dt = o.NP_SCALAR[scalar]
    shape = (n_in, 2) if cplx else (n_in,)
    if np.issubdtype(dt, np.floating):
        x = rng.uniform(-1, 1, shape).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    return x, n_in, n_out


def _fill(torch_dtype, torch, low):
    if torch_dtype.is_floating_point:
        return float("nan")
    info = torch.iinfo(torch_dtype)
    return info.min if low else info.max


def _untouched(t, fill):
    return bool(t.isnan().all()) if fill != fill else bool((t == fill).all())


def _assert_matches_oracle(row, o, scalar, got, ref, taps, x):
    exact = not np.issubdtype(o.NP_SCALAR[scalar], np.floating) or row.want == "EXACT"
    if exact:
        assert np.array_equal(got, ref), (row.name, diff_note(got, ref))
        return
    bar = row.bar if row.bar is not None else (1e-13 if scalar == o.F64 else TOL)
    # normalised by the output level (at least a tenth of the filter's typical output: one cancelling output must not set it)
    typical = float(np.sqrt(np.sum(np.abs(taps) ** 2) / row.L) * np.sqrt(np.mean(x.astype(np.float64) ** 2) * (2 if x.ndim == 2 else 1)))
    scale = max(float(np.max(np.abs(ref))), 0.1 * typical)
    err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64))))
    assert err <= bar * scale, (row.name, err / scale, bar)


def _configure(f, row, q=None):
    """the handle's settings through the setters alone"""
    from oracle import oracle as o
    from pothoscomms_amd import _lib
    f.set_taps(_taps(row))
    f.set_decimation(row.M)
    f.set_interpolation(row.L)
    f.set_algo(getattr(_lib, "FIR_" + row.algo))
    if f.scalar not in (o.F32, o.F64):          # integer element types: the Q-format reading is one more input of the tables
        f.set_qformat(q)


def _make(dev, row, q=None):
    f = dev.FirFilter(row.dtype, row.taps)
    _configure(f, row, q)
    return f


@pytest.mark.parametrize("row", PLANS, ids=IDS)
def test_plan_guard_bands_and_misaligned_windows(oracle, dev, row):
    torch, o, TD = _setup()
    from pothoscomms_amd import _lib
    d = torch.device("cuda", 0)
    f = _make(dev, row)
    scalar, cplx = f.scalar, f.is_complex
    assert f.K == _K(row)
    taps = _taps(row)
    xh, n_in, n_out = _stream(row, o, scalar, cplx)
    ref_blk = o.Fir(scalar, cplx, row.taps == "COMPLEX")
    ref_blk.set_taps(taps); ref_blk.set_decimation(row.M); ref_blk.set_interpolation(row.L); ref_blk.activate()
    ref, rc, rp, _ = ref_blk.work(xh, n_out)
    assert rp == n_out > 0, (row.name, rp, n_out)
    td, width = TD[scalar], 2 if cplx else 1
    fin, fout = _fill(td, torch, True), _fill(td, torch, False)
    first = None
    for off in (0, 1, 3):
        xw, x = guarded(torch, d, n_in, width, td, fin, off)
        yw, y = guarded(torch, d, n_out, width, td, fout, off)
        x.copy_(h2d(xh, d))
        c, p = f.process_dev(x, y, n_in, n_out)
        torch.cuda.synchronize()
        assert (c, p) == (rc, rp), (row.name, off)
        assert f.last_algo == getattr(_lib, "FIR_" + row.want), (row.name, f.last_algo)
        assert bands_intact(yw, n_out, width, fout, off), (row.name, off, "a store outside the output window")
        assert bands_intact(xw, n_in, width, fin, off), (row.name, off, "a store into the input")
        got = y.cpu().numpy()
        if td.is_floating_point:
            assert not np.isnan(got).any(), (row.name, off, "a NaN from beyond the input window, or an output left unwritten")
        if first is None:
            _assert_matches_oracle(row, o, scalar, got, ref, taps, xh)
            first = got
        else:
            assert np.array_equal(got.view(np.uint8), first.view(np.uint8)), (row.name, off, diff_note(got, first))


GATE_VALUE = 7                    # the gate word is set to it before every gated call: nothing waits on a later signal
QREADINGS = [None, (1, 1, 2)]     # the process-wide reading; half-element fraction, nearest, rounding fromQ


@pytest.mark.parametrize("kind", sorted(set((r.dtype, r.taps) for r in PLANS)), ids=lambda k: "%s-%s" % k)
def test_plans_reconfigured_on_one_handle(oracle, dev, kind):
    """one handle through every row of its stream type, three shuffled passes: each call bit-identical to a fresh handle"""
    torch, o, TD = _setup()
    d = torch.device("cuda", 0)
    rows = [r for r in PLANS if (r.dtype, r.taps) == kind]
    rng = np.random.default_rng(zlib.crc32(("%s-%s" % kind).encode()))
    walker = dev.FirFilter(*kind)
    gate = torch.full((64,), GATE_VALUE, dtype=torch.int32, device=d)
    integer = walker.scalar not in (o.F32, o.F64)
    td, width = TD[walker.scalar], 2 if walker.is_complex else 1
    fresh_out, inputs = {}, {}
    for _ in range(3):
        for i in rng.permutation(len(rows)):
            row = rows[int(i)]
            q = QREADINGS[int(rng.integers(0, 2))] if integer else None
            if row.name not in inputs:
                xh, n_in, n_out = _stream(row, o, walker.scalar, walker.is_complex)
                inputs[row.name] = (h2d(xh, d), n_in, n_out)
            x, n_in, n_out = inputs[row.name]
            _configure(walker, row, q)
            y = torch.full((n_out, width) if width > 1 else (n_out,), _fill(td, torch, False), dtype=td, device=d)
            # a call this short has no gated launch on any plan: whatever the handle ran before, nothing is queued
            assert walker.process_dev_gated(x, y, gate, GATE_VALUE, n_in, n_out) == (0, 0, False), row.name
            torch.cuda.synchronize()
            assert _untouched(y, _fill(td, torch, False)), (row.name, "an ungated call wrote its output")
            got = (walker.process_dev(x, y, n_in, n_out), walker.last_algo, y)
            key = (row.name, q)
            if key not in fresh_out:
                ff = _make(dev, row, q)
                yf = torch.full_like(y, _fill(td, torch, False))
                fresh_out[key] = (ff.process_dev(x, yf, n_in, n_out), ff.last_algo, yf)
            want = fresh_out[key]
            assert got[:2] == want[:2], (row.name, q, got[:2], want[:2])
            if not torch.equal(got[2].view(torch.uint8), want[2].view(torch.uint8)):
                g, w = got[2].cpu().numpy(), want[2].cpu().numpy()
                raise AssertionError("%s (q %s): the reconfigured handle differs from a fresh one: %s" % (row.name, q, diff_note(g, w)))


GATED_N = 2100 * 4096     # outputs of a gated call: more than 2048 blocks of the plain plan whatever K (its dealt, gated launch)


@pytest.fixture(scope="module")
def gated_buffers():
    """one input, one output and one reference buffer for every row: GATED_N elements of the widest type and room for the taps"""
    import torch
    d = torch.device("cuda", 0)
    nbytes = (GATED_N + 8200) * 16
    xin = torch.empty(nbytes // 4, dtype=torch.float32, device=d).uniform_(-1, 1, generator=torch.Generator(d).manual_seed(5))
    out = torch.empty(nbytes, dtype=torch.uint8, device=d)
    ref = torch.empty(nbytes, dtype=torch.uint8, device=d)
    gate = torch.zeros(64, dtype=torch.int32, device=d)
    gate[0] = GATE_VALUE                  # already open: nothing waits on a later signal
    torch.cuda.synchronize()
    yield xin, out, ref, gate
    del xin, out, ref, gate


SENTINEL = 0xA5


@pytest.mark.parametrize("row", PLANS, ids=IDS)
def test_plan_gated_call_contract(oracle, dev, row, gated_buffers):
    """include/pcx.h: *gated = 0 with nothing queued for everything but complex_float32, M = L = 1, K <= 2049 on the overlap-save
    plan; that one runs gated and computes what the plain call computes"""
    torch, o, TD = _setup()
    xin, out, refbuf, gate = gated_buffers
    f = _make(dev, row)
    esz = {torch.float32: 4, torch.float64: 8, torch.int64: 8, torch.int32: 4, torch.int16: 2, torch.int8: 1}[TD[f.scalar]] * (2 if f.is_complex else 1)
    cap = out.numel() // esz                          # every element count below stays inside the buffers
    K = _K(row)
    in_elems = min(cap, K - 1 + GATED_N * row.M)
    out_cap = min(cap, GATED_N)
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    c, p, gated = f.process_dev_gated(xin, out, gate, GATE_VALUE, in_elems=in_elems, out_cap=out_cap)
    torch.cuda.synchronize()
    has_gate = (row.dtype == "complex_float32" and row.L == row.M == 1 and K <= 2049 and row.want == "OLS_FFT")
    if not has_gate:
        assert (gated, c, p) == (False, 0, 0), (row.name, gated, c, p)
        assert bool((out == SENTINEL).all()), (row.name, "an ungated call wrote its output")
        return
    assert gated and (c, p) == (in_elems - (K - 1), out_cap) == (GATED_N, GATED_N), (row.name, gated, c, p)
    refbuf.fill_(SENTINEL)
    assert f.process_dev(xin, refbuf, in_elems, out_cap) == (c, p)
    torch.cuda.synchronize()
    assert torch.equal(out, refbuf), row.name
    assert bool((out[p * esz:] == SENTINEL).all()), (row.name, "a store past the produced outputs")
    assert not bool(out[:p * esz].view(torch.float32).isnan().any()), row.name


@pytest.mark.parametrize("ntaps,algo", [(2049, "AUTO"), (127, "DIRECT"), (2049, "DIRECT")])
def test_fm_chain_gated_call_without_a_gated_plan(dev, ntaps, algo, gated_buffers):
    """the fused chain has a gate only in its frequency-domain kernel (K <= 2048): the long-filter path and DIRECT queue nothing"""
    import torch

    from pothoscomms_amd import _lib
    xin, out, _, gate = gated_buffers
    ch = dev.FmChain(); ch.set_phase(0.3)
    ch.set_taps(np.random.default_rng(ntaps).normal(size=ntaps) / ntaps, False)
    ch.set_algo(getattr(_lib, "FIR_" + algo))
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    c, p, gated = ch.process_dev_gated(xin, out, gate, GATE_VALUE, GATED_N + ntaps - 1, GATED_N)
    torch.cuda.synchronize()
    assert (gated, c, p) == (False, 0, 0)
    assert bool((out == SENTINEL).all())
