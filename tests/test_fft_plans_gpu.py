"""Every plan of pcx_fft_create through one table: a higher-precision truth, impulses and tones, and the call contract.

PLANS holds the smallest sizes that reach each of the eleven plan kinds and each of their internal branches.  Every row names the
kind and the split it expects; every test asserts Fft.plan() first, so a threshold that moves in pcx_fft_create fails here instead
of silently testing another plan.  (tests/test_fft_truth_cpu.py checks the same table against a restatement of the selection.)

(a) accuracy on noise: uniform(-1, 1) frames against tests/fft_truth.py (numpy's float64 transform for complex_float32, the
    long-double transform for complex_float64 up to 2^17 bins).  The device's worst per-frame relative L2 error must not exceed
    FACTOR * max(E_ref, 4 u): E_ref is the oracle's worst per-frame error on the same input against the same truth, u the unit
    roundoff of the type.  No bar is taken from the device's output.
(b) impulses at p in {0, 1, N/3, N-1} and unit tones at k in {1, N/3, N-1}: every bin of an impulse's transform is a bare twiddle,
    a tone's transform is one line and what leaks from it.  Same form of bar, E_ref the oracle's worst over the same frames (the
    chirp-z plan's impulses carry a factor of their own, IMPULSE_FACTOR, with the count of roundings behind it).  An
    impulse at p = 0 must give exactly 1.0 in every bin on every plan but the chirp-z one, whose convolution rounds (DC_EXACT).
(c) the contract of pcx_fft_transform_dev: windows that are element-aligned only, inside poisoned buffers; in place; one handle
    over growing and shrinking frame counts with a handle of the other direction in between; a stream of the caller's.  All bit
    for bit against the plain call, which itself meets the bar of (a) (complex_int16: equals the oracle).

Frames: 3 a call, 37 below 256 bins (the last workgroup's group of frames is ragged), 1 above 2^20 bins (there also two impulses
and one tone instead of four and three).
"""
import collections
import zlib

import numpy as np
import pytest

from tests import fft_truth as ft
from tests.util import bands_intact, diff_note, guarded, h2d

pytestmark = pytest.mark.gpu

Row = collections.namedtuple("Row", "dtype nbins kind n1 n2")
F32, F64, I16 = "complex_float32", "complex_float64", "complex_int16"


def _rows(dtype, kind, sizes):
    return [Row(dtype, s[0], kind, s[1], s[2]) if isinstance(s, tuple) else Row(dtype, s, kind, 0, 0) for s in sizes]


PLANS = (
    # -- complex_float32: one workgroup to 16384 bins (powers of two) / 10240 bins (the ping-pong image in LDS) --
    _rows(F32, "IDENTITY", [1])
    + _rows(F32, "POW2", [2, 4, 8])
    # 16 ... 64: staged I/O, several frames a workgroup; 128: the first size past it; log2 N mod 4 = 0, 1, 2, 3, 3, 2
    + _rows(F32, "R16", [16, 32, 64, 128, 2048, 16384])
    + _rows(F32, "R16_4096", [4096])
    # radix 6 alone; 15 x 3; 9 x 9; 16 x 15 x 3; 8 x 5 x 5 x 5; 16 x 16 x 2 x 15
    + _rows(F32, "SMOOTH", [6, 45, 81, 720, 1000, 7680])
    # 10000 is 5-smooth, from 8192 bins up in kissfft's order; 10223 is the largest prime that fits one workgroup
    + _rows(F32, "MIXED", [7, 77, 1001, 10000, 10223])
    # rows transposed on the store (n2 <= 256) at 2^15 and 2^16; a sub-plan of n2 bins and one transpose beyond
    + _rows(F32, "FOURSTEP_SHORT", [(1 << 15, 128, 256), (1 << 16, 256, 256), (1 << 17, 128, 1024), (1 << 22, 256, 16384)])
    # five passes at 2^23; the composite 100 x 120; 2 x a prime that fits; 2 3 5 7 11 13
    + _rows(F32, "FOURSTEP", [(1 << 23, 4096, 2048), (12000, 100, 120), (2 * 10223, 2, 10223), (30030, 165, 182)])
    # M = 32768 and 65536: the sub-plans are themselves FOURSTEP_SHORT
    + _rows(F32, "BLUESTEIN", [(10243, 10243, 32768), (2 * 10243, 2 * 10243, 65536)])
    # -- complex_float64: one workgroup to 8192 bins (powers of two) / 5120 bins --
    + _rows(F64, "IDENTITY", [1])
    + _rows(F64, "POW2", [2, 4, 8])
    + _rows(F64, "R16", [16, 64, 4096, 8192])
    + _rows(F64, "SMOOTH", [300, 1125, 1536])
    + _rows(F64, "MIXED", [60, 243, 77, 3000, 5119])
    + _rows(F64, "FOURSTEP_SHORT", [(1 << 14, 128, 128), (1 << 15, 128, 256), (1 << 17, 128, 1024), (1 << 21, 256, 8192)])
    + _rows(F64, "FOURSTEP", [(1 << 22, 2048, 2048), (12000, 100, 120)])
    + _rows(F64, "BLUESTEIN", [(5147, 5147, 16384)])
    # -- complex_int16, for the contract tests only: its arithmetic is bit-exact against the oracle --
    + _rows(I16, "IDENTITY", [1])
    + _rows(I16, "Q15_POW2", [64, 1024, 4096])
    + _rows(I16, "MIXED", [60, 1000])
    + _rows(I16, "Q15_GLOBAL", [65536, 40000])
)

# FACTOR * max(E_ref, 4 u) is the bar.  2 for every plan: the device takes its radices in another order than kissfft (16s first), so
# equal quality does not mean equal roundings, but a plan twice as bad as kissfft on the same input is a defect.  A plan may carry
# another factor only with the count of its extra roundings written down in DESIGN.md ("FFT accuracy").
FACTOR = {kind: 2 for kind in ("IDENTITY", "R16_4096", "R16", "POW2", "MIXED", "SMOOTH", "FOURSTEP", "FOURSTEP_SHORT", "BLUESTEIN")}
# impulses through the chirp-z plan, DESIGN.md "FFT accuracy": kissfft's generic butterfly gives each bin of an impulse's transform
# as ONE product, so its error there is that of one twiddle (6 u at 5147 bins in double), while the device's bin has been through three
# M-point transforms (M = 16384: 12 u each on an impulse, no worse than kissfft's own 17 u at that size; sqrt(3) x 12 u = 21 u) and two
# chirp products.  Measured 19.9 u, 3.21 x max(E_ref, 4 u); the factor is the smallest integer not below 1.5 x that.
IMPULSE_FACTOR = dict(FACTOR, BLUESTEIN=5)
# an impulse at sample 0 meets only the twiddle 1 + 0j on its way, in every plan but the chirp-z one
DC_EXACT = frozenset(FACTOR) - {"BLUESTEIN"}

NP_DT = {F32: np.float32, F64: np.float64, I16: np.int16}
INT16_POISON = 12345


def row_id(row):
    return "%s-%d-%s" % (row.dtype.replace("complex_", "c"), row.nbins, row.kind)


def frames_of(row):
    return 1 if row.nbins > 1 << 20 else 37 if row.nbins < 256 else 3


def has_truth(row):
    """float rows with a truth for noise: float64 for complex_float32, long double for complex_float64 up to 2^17 bins"""
    return row.dtype == F32 or (row.dtype == F64 and row.nbins <= ft.LD_LIMIT)


def noise(row, inverse, nframes=None, salt=0):
    """the row's seeded input: uniform(-1, 1) pairs of the device type (any int16 for complex_int16)"""
    nf = frames_of(row) if nframes is None else nframes
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d/%d" % (row.dtype, row.nbins, int(inverse), salt)).encode()))
    if row.dtype == I16:
        return rng.integers(-32768, 32768, (nf * row.nbins, 2)).astype(np.int16)
    return rng.uniform(-1, 1, (nf * row.nbins, 2)).astype(NP_DT[row.dtype])


def truth_of(row, x, inverse):
    return (ft.truth64 if row.dtype == F32 else ft.truth_ld)(x, row.nbins, inverse)


def impulses(row):
    """(positions, input): unit impulses at 0, 1, N // 3, N - 1 (those that differ), one frame each; above 2^20 bins at 0 and
    N // 3 only (the frames are cut there, not the size: the oracle takes over a second a frame)"""
    n = row.nbins
    ps = sorted(set(p % n for p in ((0, 1, n // 3, n - 1) if n <= 1 << 20 else (0, n // 3))))
    x = np.zeros((len(ps), n, 2), NP_DT[row.dtype])
    for f, p in enumerate(ps):
        x[f, p, 0] = 1
    return ps, x.reshape(-1, 2)


def tone_bins(row):
    """tones at bins 1, N // 3, N - 1 (those that differ); above 2^20 bins at N // 3 only"""
    n = row.nbins
    return sorted(set(k % n for k in ((1, n // 3, n - 1) if n <= 1 << 20 else (n // 3,))))


FLOAT_ROWS = [r for r in PLANS if r.dtype != I16]
ACC_CASES = [(r, inv) for r in FLOAT_ROWS if has_truth(r) for inv in (False, True)]
FLOAT_CASES = [(r, inv) for r in FLOAT_ROWS for inv in (False, True)]
ALL_CASES = [(r, inv) for r in PLANS for inv in (False, True)]


def case_id(case):
    return row_id(case[0]) + ("-inv" if case[1] else "-fwd")


def _torch():
    import torch
    return torch, torch.device("cuda", 0), {F32: torch.float32, F64: torch.float64, I16: torch.int16}


def _need_long_double(row):
    if row.dtype == F64 and not ft.LD_IS_EXTENDED:
        pytest.skip("numpy.longdouble is no wider than float64 here (eps %.3g): no truth for complex_float64" % ft.LD_EPS)


def _open(dev, row, inverse):
    """the row's handle, which must be on the plan the row names"""
    f = dev.Fft(row.dtype, row.nbins, inverse)
    assert f.plan() == (row.kind, row.n1, row.n2), (row_id(row), f.plan())
    return f


def _run(f, x, nframes):
    """one plain call on fresh device buffers: host pairs in, host pairs out"""
    torch, d, _ = _torch()
    xd = h2d(x, d)
    yd = torch.empty_like(xd)
    f.transform_dev(xd, yd, nframes)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view(torch.uint8)


_BARS = {}


def noise_reference(oracle, row, inverse):
    """(x, nframes, truth, bar) of the row's noise input; truth and bar are None where (a) does not apply.  E_ref is computed once
    per case and kept (a number); the arrays are kept only where they are small."""
    key = (row, inverse)
    nf = frames_of(row)
    hit = _BARS.get(key)
    if hit is not None and hit[0] is not None:
        return hit
    x = noise(row, inverse)
    if row.dtype == I16 or not has_truth(row):
        return x, nf, None, None, None
    truth = truth_of(row, x, inverse)
    e_ref = hit[4] if hit is not None else float(np.max(ft.rel_l2(oracle.fft(x, row.nbins, inverse), truth, row.nbins)))
    out = (x, nf, truth, ft.bar(e_ref, ft.UNIT[row.dtype], FACTOR[row.kind]), e_ref)
    _BARS[key] = out if nf * row.nbins <= 1 << 16 else (None, nf, None, out[3], e_ref)
    return out


def _report(what, row, inverse, err, e_ref, u, b):
    print("FFTACC %-8s %s %-3s err %.3g u  E_ref %.3g u  bar %.3g u  err/max(E_ref,4u) %.3f" % (
        what, row_id(row), "inv" if inverse else "fwd", err / u, e_ref / u, b / u, err / max(e_ref, 4 * u)))


# ---- (a) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACC_CASES, ids=case_id)
def test_accuracy_on_noise(oracle, dev, case):
    row, inverse = case
    _need_long_double(row)
    f = _open(dev, row, inverse)
    x, nf, truth, b, e_ref = noise_reference(oracle, row, inverse)
    got = _run(f, x, nf)
    err = float(np.max(ft.rel_l2(got, truth, row.nbins)))
    _report("noise", row, inverse, err, e_ref, ft.UNIT[row.dtype], b)
    assert err <= b, (row_id(row), inverse, "rel L2 %.3g, oracle %.3g, bar %.3g" % (err, e_ref, b))


# ---- (b) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FLOAT_CASES, ids=case_id)
def test_impulses(oracle, dev, case):
    row, inverse = case
    _need_long_double(row)
    f = _open(dev, row, inverse)
    u, n = ft.UNIT[row.dtype], row.nbins
    ps, x = impulses(row)
    got = _run(f, x, len(ps)).reshape(len(ps), n, 2)
    ref = oracle.fft(x, n, inverse).reshape(len(ps), n, 2)
    err = e_ref = 0.0
    for i, p in enumerate(ps):
        truth = ft.impulse_truth(n, p, inverse)
        err = max(err, ft.impulse_err(got[i], truth, n))
        e_ref = max(e_ref, ft.impulse_err(ref[i], truth, n))
    b = ft.bar(e_ref, u, IMPULSE_FACTOR[row.kind])
    _report("impulse", row, inverse, err, e_ref, u, b)
    dc_exact = bool(np.all(got[0, :, 0] == 1) and np.all(got[0, :, 1] == 0))
    print("FFTDC %s %s exact %s" % (row_id(row), "inv" if inverse else "fwd", dc_exact))
    assert err <= b, (row_id(row), inverse, "impulse error %.3g, oracle %.3g, bar %.3g" % (err, e_ref, b))
    if row.kind in DC_EXACT:
        assert dc_exact, (row_id(row), inverse, "an impulse at sample 0 is not exactly 1 in every bin",
                          float(np.max(np.abs(got[0] - np.array([1, 0])))))


@pytest.mark.parametrize("case", FLOAT_CASES, ids=case_id)
def test_tones(oracle, dev, case):
    row, inverse = case
    _need_long_double(row)
    f = _open(dev, row, inverse)
    u, n = ft.UNIT[row.dtype], row.nbins
    ks = tone_bins(row)
    pairs = [ft.tone(n, k, NP_DT[row.dtype], inverse) for k in ks]
    x = np.concatenate([p[0] for p in pairs])
    got = _run(f, x, len(ks)).reshape(len(ks), n, 2)
    ref = oracle.fft(x, n, inverse).reshape(len(ks), n, 2)
    err = max(ft.tone_leak(got[i], pairs[i][1], n) for i in range(len(ks)))
    e_ref = max(ft.tone_leak(ref[i], pairs[i][1], n) for i in range(len(ks)))
    b = ft.bar(e_ref, u, FACTOR[row.kind])
    _report("tone", row, inverse, err, e_ref, u, b)
    assert err <= b, (row_id(row), inverse, "tone leakage %.3g, oracle %.3g, bar %.3g" % (err, e_ref, b))


# ---- (c) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_misaligned_windows_and_guard_bands(oracle, dev, case):
    """element offset 1 puts a window 8 (complex_float32), 16 (complex_float64) or 4 (complex_int16) bytes off its alignment"""
    row, inverse = case
    if has_truth(row):
        _need_long_double(row)
    torch, d, TD = _torch()
    f = _open(dev, row, inverse)
    ref = noise_reference(oracle, row, inverse)
    x, nf, truth = ref[0], ref[1], ref[2]
    n_elems = nf * row.nbins
    poison = INT16_POISON if row.dtype == I16 else float("nan")
    xd = h2d(x, d)
    first = None
    for off in (0, 1):
        xw, xin = guarded(torch, d, n_elems, 2, TD[row.dtype], poison, off)
        yw, y = guarded(torch, d, n_elems, 2, TD[row.dtype], poison, off)
        xin.copy_(xd)
        before = _bits(xw).clone()
        f.transform_dev(xin, y, nf)
        torch.cuda.synchronize()
        assert bands_intact(yw, n_elems, 2, poison, off), (row_id(row), off, "a store outside the output window")
        assert torch.equal(_bits(xw), before), (row_id(row), off, "a store into the input buffer")
        got = y.cpu().numpy()
        if first is None:
            first = got
            if row.dtype == I16:
                want = oracle.fft(x, row.nbins, inverse)
                assert np.array_equal(got, want), (row_id(row), diff_note(got, want))
            elif truth is not None:
                err = float(np.max(ft.rel_l2(got, truth, row.nbins)))
                assert err <= ref[3], (row_id(row), inverse, "rel L2 %.3g, bar %.3g" % (err, ref[3]))
            else:
                assert not np.isnan(got).any(), row_id(row)
        else:
            assert np.array_equal(got.view(np.uint8), first.view(np.uint8)), (row_id(row), off, diff_note(got, first))


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_in_place(dev, case):
    """out == in (include/pcx.h) computes what the same handle computes out of place"""
    row, inverse = case
    torch, d, _ = _torch()
    f = _open(dev, row, inverse)
    nf = frames_of(row)
    x = h2d(noise(row, inverse), d)
    y = torch.empty_like(x)
    f.transform_dev(x, y, nf)
    t = x.clone()
    f.transform_dev(t, t, nf)
    torch.cuda.synchronize()
    assert torch.equal(_bits(t), _bits(y)), (row_id(row), diff_note(t.cpu().numpy(), y.cpu().numpy()))


def _device_noise(torch, d, row, nframes, seed):
    g = torch.Generator(d).manual_seed(seed)
    shape = (nframes * row.nbins, 2)
    if row.dtype == I16:
        return torch.randint(-32768, 32768, shape, dtype=torch.int16, device=d, generator=g)
    return torch.empty(shape, dtype=torch.float32 if row.dtype == F32 else torch.float64, device=d).uniform_(-1, 1, generator=g)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_handle_reuse_over_frame_counts(dev, case):
    """one handle over growing, then shrinking frame counts (the workspace plans size their buffers per call and hand
    nframes * n1 frames to their sub-plans), a handle of the other direction on the same size between the calls: every call
    bit for bit what a fresh handle computes"""
    row, inverse = case
    torch, d, _ = _torch()
    f = _open(dev, row, inverse)
    other = _open(dev, row, not inverse)
    counts = (37, 300, 1) if row.nbins < 256 else (1, 5, 2)
    for i, nf in enumerate(counts):
        x = _device_noise(torch, d, row, nf, 1000 * i + nf)
        y, scratch, want = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        f.transform_dev(x, y, nf)
        other.transform_dev(x, scratch, nf)
        _open(dev, row, inverse).transform_dev(x, want, nf)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(want)), (row_id(row), "call %d, %d frames" % (i, nf), diff_note(y.cpu().numpy(), want.cpu().numpy()))
        del x, y, scratch, want


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_callers_stream(dev, case):
    """one call on a stream of the caller's, only that stream synchronised, equals the default-stream call"""
    row, inverse = case
    torch, d, _ = _torch()
    f = _open(dev, row, inverse)
    nf = frames_of(row)
    x = h2d(noise(row, inverse), d)
    y, ys = torch.empty_like(x), torch.zeros_like(x)
    f.transform_dev(x, y, nf)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=d)
    f.transform_dev(x, ys, nf, stream=side)
    side.synchronize()
    assert torch.equal(_bits(ys), _bits(y)), (row_id(row), diff_note(ys.cpu().numpy(), y.cpu().numpy()))
