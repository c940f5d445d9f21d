"""The overlap-save inverse on the folded butterflies (pothoscomms_amd/csrc/fft4096.hpp: fft4_fold, ols_block.hpp:
spectrum_times_h_inner): the complex_float32 4096-sample kernels and the fused chain, which took the fold.

A butterfly whose second operand carries a multiplier is p = a + w b by two chained multiply-adds and q = 2 a - p; the H multiply rides on
the inner layer of the inverse's first sixteen-point transform in the same way.  Every chain is written out with its own operand
selects and signs, sixteen registers a lane, three transforms a block.  What the tests below are for:

- every bin's path: sixteen unit tones whose three radix-16 index digits each take all sixteen values through a pure delay.  A wrong
  select or sign in ONE register's chain of ONE pass corrupts one tone at full size (an error of the order of max|x|, 10^6 times the bar);
- the dealt form of the same kernel (taken above 2048 blocks) on noise, windows at the head, at a block seam, mid-stream and the ragged tail;
- the other ends of the overlap ladder, K = 2 (row 0 partly stored) and K = 2049 (eight rows dropped);
- the fused chain, three blocks, against the oracle as tests/test_parity_gpu.py::test_fm_chain holds it.

Bars come from tests/fir_truth.py as the truth tests take them: twice the plain overlap-save's figure on the same input against the same
wider truth, floors 4 u (l2, and the tone test's absolute error) and 16 u (mx).  None comes from the device's output.  Every case prints
its figures (OLSFOLD lines, in u) before it asserts.
"""
import numpy as np
import pytest

from tests import fir_plans as fp
from tests import fir_truth as ft
from tests.util import TOL, ang_err, h2d

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _row(name, ntaps, taps="COMPLEX"):
    return fp.R(name, "complex_float32", taps, ntaps, plan="CF32_OLS4096")


def _run(dev, row, taps, x, n_in, n_out):
    import torch
    d = torch.device("cuda", 0)
    f = dev.FirFilter(row.dtype, row.taps)
    f.set_taps(taps)
    y = torch.full((n_out, 2), float("nan"), dtype=torch.float32, device=d)
    c, p = f.process_dev(h2d(x, d), y, n_in, n_out)
    torch.cuda.synchronize()
    assert p == n_out, (row.name, c, p, n_out)
    assert f.last_plan == row.plan, (row.name, f.last_plan, row.plan)
    got = y.cpu().numpy()
    assert not np.isnan(got).any(), (row.name, "an output left unwritten")
    return got


def _pairs(z):
    return np.ascontiguousarray(np.stack([z.real.astype(np.float32), z.imag.astype(np.float32)], axis=1))


def test_every_bin_through_the_inverse(oracle, dev):
    """two full blocks and a ragged one on the grid-stride kernel; the output is the input, 254 samples late"""
    K, n_out = 255, 2 * 3840 + 17
    row = _row("fold tones K=255", K, "REAL")
    taps = np.zeros(K); taps[K - 1] = 1.0
    i = np.arange(16)
    ks = i + 16 * ((5 * i + 3) % 16) + 256 * ((11 * i + 7) % 16)
    for digit in (ks % 16, (ks // 16) % 16, ks // 256):
        assert sorted(digit.tolist()) == list(range(16))
    n_in = K - 1 + n_out
    n = np.arange(n_in, dtype=np.float64)
    x = _pairs(np.sum(np.exp(2j * np.pi * np.outer(ks, n) / 4096), axis=0))
    t = ft.truth(row, taps, x, n_out)
    assert np.array_equal(t, ft.as_complex(x[:n_out], np.float64, np.complex128))      # y[i] = x[K - 1 + i - 254] = x[i], exactly
    xmax = float(np.max(np.abs(ft.as_complex(x, np.float64, np.complex128))))
    e_plain = ft.max_abs_err(row, ft.plain_ols(row, taps, x, n_out), t) / U / xmax
    got = _run(dev, row, taps, x, n_in, n_out)
    err = ft.max_abs_err(row, got, t) / U / xmax
    bar = ft.FACTOR * max(e_plain, ft.FLOOR_L2)
    print("OLSFOLD tones | err %.3g | E_plain %.3g | bar %.3g | ratio %.2f" % (err, e_plain, bar, err / bar))
    assert err <= bar, (err, bar)


def _noise_case(oracle, dev, row, n_out, windows, seed):
    """random taps and stream; each window of outputs against the truth of its own slice of the input, bars from plain_ols on that slice"""
    K = row.ntaps
    rng = np.random.default_rng(seed)
    taps = (rng.normal(size=K) + 1j * rng.normal(size=K)) * 0.9 / np.sqrt(K)
    n_in = K - 1 + n_out
    x = rng.uniform(-1, 1, (n_in, 2)).astype(np.float32)
    got = _run(dev, row, taps, x, n_in, n_out)
    worst = 0.0
    for s, m in windows:
        xs = x[s:s + m + K - 1]
        t = ft.truth(row, taps, xs, m)
        e_plain = ft.l2_mx(row, ft.plain_ols(row, taps, xs, m), t)
        l2, mx = ft.l2_mx(row, got[s:s + m], t)
        bar_l2, bar_mx = ft.bars(row, None, e_plain)
        print("OLSFOLD noise | %s | outputs %d..%d | l2 %.3g of %.3g | mx %.3g of %.3g | E_plain %.3g %.3g | ratio %.2f" % (
            row.name, s, s + m, l2, bar_l2, mx, bar_mx, e_plain[0], e_plain[1], max(l2 / bar_l2, mx / bar_mx)))
        worst = max(worst, l2 / bar_l2, mx / bar_mx)
    assert worst <= 1.0, (row.name, worst)


def test_dealt_kernel_on_the_same_stream(oracle, dev):
    """above 2048 blocks the handle's calls are dealt: the other instantiation of the same kernel"""
    S, n_out = 3840, 2050 * 3840 + 5
    windows = [(0, 4096), (2 * S - 2048, 4096), (1025 * S - 1000, 4096), (n_out - 4096, 4096)]
    _noise_case(oracle, dev, _row("fold dealt K=255", 255), n_out, windows, 20255)


@pytest.mark.parametrize("K,S", [(2, 4080), (2049, 2048)])
def test_ends_of_the_overlap_ladder(oracle, dev, K, S):
    """three blocks, the last ragged: K = 2 stores all but sixteen samples of row 0, K = 2049 drops eight rows whole"""
    n_out = 2 * S + 17
    _noise_case(oracle, dev, _row("fold K=%d" % K, K), n_out, [(0, n_out)], 30000 + K)


def test_fused_chain_three_blocks(oracle, dev):
    """Rotate -> FIR (127 real taps) -> FreqDemod in one kernel: blocks of 3968 outputs, two full and one ragged, against the three
    reference blocks back to back at the parity bar"""
    from pothoscomms_amd import taps as tp
    ntaps = 127
    n = 2 * 3968 + 17 + ntaps - 1
    x = tp.fm_test_signal(n)
    taps = tp.lowpass(ntaps, 0.1)
    xr = oracle.rotate(x, 0.7)
    fir = oracle.Fir(oracle.F32, True, False); fir.set_taps(taps); fir.activate()
    y, _, _, _ = fir.work(xr, n)
    ref = oracle.FreqDemod(oracle.F32).work(y)
    ch = dev.FmChain(); ch.set_phase(0.7); ch.set_taps(taps, False)
    ch.set_algo(dev._lib.FIR_OLS_FFT)
    got, c, p = ch.process(x, n)
    assert (c, p) == (n - ntaps + 1, n - ntaps + 1)
    assert ch.last_algo == dev._lib.FIR_OLS_FFT
    err = ang_err(got, ref)
    print("OLSFOLD chain | err %.3g of pi | bar %.3g" % (err, TOL))
    assert err <= TOL
