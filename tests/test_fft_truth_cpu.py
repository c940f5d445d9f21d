"""CPU suite: the truth that tests/test_fft_plans_gpu.py holds the FFT plans to, the oracle's own distance from it, and that table's
plan column.

1. truth_ld (tests/fft_truth.py) against a 40-digit mpmath DFT at 8, 12, 31 and 64 bins and against the direct long-double DFT at
   1000 bins, within 64 eps of long double: a chirp reduced modulo the wrong period, or a twiddle from an unreduced index, misses it.
2. the oracle, float32 and float64, at every size of the table up to 2^17 bins on the table's own inputs -- noise, impulses, tones --
   inside oracle_cap(N): E_ref in the bars of the GPU test is the oracle's error, so a bar there is at most FACTOR * that cap, and a
   device plan that matches the oracle's quality passes whatever the oracle's roundings were.
3. every row's plan kind and split equal what a restatement of pcx_fft_create's selection gives.  (On the GPU Fft.plan() decides.)
"""
import numpy as np
import pytest

from tests import fft_truth as ft
from tests import test_fft_plans_gpu as table

needs_long_double = pytest.mark.skipif(not ft.LD_IS_EXTENDED, reason="numpy.longdouble is no wider than float64 here (eps %.3g): "
                                       "the long-double truth would be no truth" % ft.LD_EPS)
LD_BAR = 64 * ft.LD_EPS


def _mp_dft(x, inverse):
    """the DFT of one frame of float64 pairs in 40 digits, as a long-double array (high part + remainder)"""
    import mpmath
    mpmath.mp.dps = 40
    n = len(x)
    xs = [mpmath.mpc(float(re), float(im)) for re, im in x]
    sign = 1 if inverse else -1
    w = [mpmath.expjpi(mpmath.mpf(sign * 2 * j) / n) for j in range(n)]
    out = np.empty(n, dtype=ft.CLD)
    for k in range(n):
        s = mpmath.fsum(xs[i] * w[(k * i) % n] for i in range(n))
        parts = []
        for v in (s.real, s.imag):
            hi = float(v)
            parts.append(ft.LD(hi) + ft.LD(float(v - hi)))
        out[k] = parts[0] + ft.CLD(1j) * parts[1]
    return out


@needs_long_double
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("nbins", [8, 12, 31, 64])
def test_truth_ld_against_mpmath(nbins, inverse):
    x = np.random.default_rng(nbins).uniform(-1, 1, (nbins, 2))
    want = _mp_dft(x, inverse)
    assert float(ft.rel_l2(ft.truth_ld(x, nbins, inverse), want, nbins)[0]) <= LD_BAR
    assert float(ft.rel_l2(ft.direct_ld(x, nbins, inverse), want, nbins)[0]) <= LD_BAR
    # and the float64 truth of the float32 plans, at its own precision
    assert float(ft.rel_l2(ft.truth64(x, nbins, inverse), want, nbins)[0]) <= 64 * 2.0 ** -53


@needs_long_double
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_truth_ld_chirp_against_direct_dft_at_1000_bins(inverse):
    x = np.random.default_rng(1000).uniform(-1, 1, (2 * 1000, 2))
    assert float(np.max(ft.rel_l2(ft.truth_ld(x, 1000, inverse), ft.direct_ld(x, 1000, inverse), 1000))) <= LD_BAR


@needs_long_double
def test_impulse_and_tone_closed_forms():
    """the O(N) truths against the transform they stand for"""
    for n, inverse in ((12, False), (64, True), (1000, False)):
        for p in (0, 1, n // 3, n - 1):
            x = np.zeros((n, 2)); x[p, 0] = 1
            assert ft.impulse_err(ft.impulse_truth(n, p, inverse), ft.truth_ld(x, n, inverse), n) <= LD_BAR
        for k in (1, n // 3, n - 1):
            for dt in (np.float32, np.float64):
                x, truth = ft.tone(n, k, dt, inverse)
                assert x.dtype == dt and ft.tone_leak(truth, ft.truth_ld(x, n, inverse), n) <= LD_BAR
                line = (-k) % n if inverse else k
                assert abs(truth[line] - n) <= 8 * n * np.finfo(dt).eps and np.max(np.abs(np.delete(truth, line))) <= 8 * n * np.finfo(dt).eps


CPU_CASES = [c for c in table.ACC_CASES if c[0].nbins <= ft.LD_LIMIT]


@pytest.mark.parametrize("case", CPU_CASES, ids=table.case_id)
def test_oracle_is_inside_its_cap(oracle, case):
    row, inverse = case
    if row.dtype == table.F64 and not ft.LD_IS_EXTENDED:
        pytest.skip("numpy.longdouble is no wider than float64 here (eps %.3g)" % ft.LD_EPS)
    n, u = row.nbins, ft.UNIT[row.dtype]
    cap = ft.oracle_cap(n, u)
    x = table.noise(row, inverse)
    e_noise = float(np.max(ft.rel_l2(oracle.fft(x, n, inverse), table.truth_of(row, x, inverse), n)))
    ps, xi = table.impulses(row)
    ref = oracle.fft(xi, n, inverse).reshape(len(ps), n, 2)
    e_imp = max(ft.impulse_err(ref[i], ft.impulse_truth(n, p, inverse), n) for i, p in enumerate(ps))
    e_tone = 0.0
    for k in table.tone_bins(row):
        xt, truth = ft.tone(n, k, table.NP_DT[row.dtype], inverse)
        e_tone = max(e_tone, ft.tone_leak(oracle.fft(xt, n, inverse), truth, n))
    print("ORACLE %s %s noise %.3g u  impulse %.3g u  tone %.3g u  cap %.3g u" % (
        table.row_id(row), "inv" if inverse else "fwd", e_noise / u, e_imp / u, e_tone / u, cap / u))
    assert e_noise <= cap and e_imp <= cap and e_tone <= cap, (table.row_id(row), e_noise / u, e_imp / u, e_tone / u, cap / u)


def test_table_names_the_plan_the_selection_gives():
    kinds = set()
    for row in table.PLANS:
        assert ft.select_plan(row.dtype, row.nbins) == (row.kind, row.n1, row.n2), (table.row_id(row), ft.select_plan(row.dtype, row.nbins))
        kinds.add(row.kind)
    from pothoscomms_amd import _lib
    assert kinds == set(_lib.FFT_PLANS)                 # every plan kind of the handle has a row
    assert len(set((r.dtype, r.nbins) for r in table.PLANS)) == len(table.PLANS)


def test_plan_constants_follow_the_header():
    import os
    import re

    from pothoscomms_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcx.h")).read()
    declared = dict((name, int(v)) for name, v in re.findall(r"PCX_FFT_PLAN_(\w+)\s*=\s*(\d+)", src))
    assert declared == {name: i for i, name in enumerate(_lib.FFT_PLANS)}
