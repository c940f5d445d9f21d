"""CPU suite: the truth that tests/test_fir_truth_gpu.py holds the float FIR plans to, the two figures its bars are built from, and
the plan column of the shared table (tests/fir_plans.py).

1. truth and impulse_truth (tests/fir_truth.py) against the exact rational sum at K = 1, 3, 16 and (L, M) = (1, 1), (3, 2), (2, 3), all
   four float stream types, within 4 eps of the wide type relative to sum |h| |x|: an index of the polyphase rule off by one misses it.
2. the oracle within 1e-5 of the truth on every float row of the table: the truth's indexing is the reference's.
3. the caps that keep the GPU bars meaningful, on every float row: the oracle's error E_ref inside (1 + sqrt K) u in l2 and
   6 (1 + sqrt K) u in mx (a sequential sum of K terms measures 0.3 sqrt K u), the plain overlap-save's E_plain inside 16 u and 48 u
   (it measures 3 ... 6 u whatever K; 14 u on the three outputs of the M = 65535 row).  A bar is at most twice a cap.
4. every row's plan is a name of _lib.FIR_PLANS, the names follow include/pcx.h, and every plan a call can report has a row.
5. the bars can fail: a truth degraded on the host by 12.5 u rms of noise, or in one sample by 1e-4 of the rms, is over them.

The float64 rows need a long double wider than double and skip, with the reason, where numpy has none.
"""
import fractions
import os
import re

import numpy as np
import pytest

from tests import fir_plans as fp
from tests import fir_truth as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_REASON = "numpy.longdouble is no wider than float64 here (eps %.3g): there is no truth for a float64 stream" % ft.LD_EPS


def _skip_without_long_double(row):
    if ft.needs_long_double(row) and not ft.LD_IS_EXTENDED:
        pytest.skip(LD_REASON)


def _frac(v):
    """a float, numpy float32 / float64 or long double as an exact Fraction (a long double as its double part plus the remainder)"""
    hi = float(v)
    return fractions.Fraction(hi) + fractions.Fraction(float(v - type(v)(hi))) if isinstance(v, ft.LD) else fractions.Fraction(hi)


def _cfrac(v):
    return (_frac(v.real), _frac(v.imag)) if np.iscomplexobj(v) else (_frac(v), fractions.Fraction(0))


EXACT_CASES = [(dtype, K, L, M) for dtype in ft.FLOAT_DTYPES for K in (1, 3, 16) for (L, M) in ((1, 1), (3, 2), (2, 3))]


@pytest.mark.parametrize("dtype,K,L,M", EXACT_CASES, ids=lambda v: str(v))
def test_truth_against_the_exact_sum(dtype, K, L, M):
    cplx = dtype.startswith("complex")
    ntaps = (K - 1) * L + 1                       # the rows after the first are one tap short: K = ceil(ntaps / L)
    row = fp.R("exact %s K=%d L=%d M=%d" % (dtype, K, L, M), dtype, "COMPLEX" if cplx else "REAL", ntaps, L=L, M=M)
    _skip_without_long_double(row)
    assert fp._K(row) == K
    rng = np.random.default_rng(K * 100 + L * 10 + M)
    taps = rng.normal(size=ntaps) + (1j * rng.normal(size=ntaps) if cplx else 0)
    it = 36 * M
    n_in, n_out = K - 1 + it, (it // M) * L
    dt = ft.np_dtype(row)
    x = rng.uniform(-1, 1, (n_in, 2) if cplx else (n_in,)).astype(dt)
    got = ft.truth(row, taps, x, n_out)
    h = ft.rounded_taps(row, taps)
    assert h.dtype == (np.dtype(dt) if not cplx else np.dtype(np.complex64 if dt == np.float32 else np.complex128))
    hf = [_cfrac(v) for v in h]
    xf = [_cfrac(v) for v in ft.as_complex(x, np.float64, np.complex128)]
    eps = float(np.finfo(got.real.dtype).eps)
    assert got.size == n_out >= 36
    for i in range(n_out):
        q = i * M + M - 1
        n, j = q // L, q % L
        re = im = mag = fractions.Fraction(0)
        for k in range(K):
            if j + k * L >= ntaps:
                continue
            (a, b), (c, d) = hf[j + k * L], xf[K - 1 + n - k]
            re += a * c - b * d
            im += a * d + b * c
            mag += fractions.Fraction(abs(complex(h[j + k * L]))) * fractions.Fraction(abs(complex(xf[K - 1 + n - k][0], xf[K - 1 + n - k][1])))
        gr, gi = _cfrac(got[i])
        err = float(abs(gr - re)) + float(abs(gi - im))
        assert err <= 4 * eps * float(mag), (i, err, float(mag), eps)
    # and the closed form for an impulse: the same function on the impulse's input
    for p in (0, 1, 7):
        xi = ft.impulse_input(row, x, p)
        assert xi.dtype == x.dtype and xi.shape == x.shape and float(np.sum(np.abs(xi))) == 1.0
        assert np.array_equal(ft.impulse_truth(row, taps, p, n_out), ft.truth(row, taps, xi, n_out)), p


@pytest.mark.parametrize("row", ft.FLOAT_ROWS, ids=[r.name for r in ft.FLOAT_ROWS])
def test_oracle_and_plain_overlap_save_inside_their_caps(oracle, row):
    _skip_without_long_double(row)
    f = ft.noise_figures(row)
    K = fp._K(row)
    # the truth's indexing is the reference's: the oracle, whose only difference is its precision, lies within the parity bar of it
    ref = ft.oracle_fir(row, f.taps, f.x, f.n_out)
    assert ft.max_abs_err(row, ref, f.t) <= 1e-5 * float(np.max(np.abs(f.t))), row.name
    cap_l2, cap_mx = ft.ref_caps(K)
    print("FIRCAP %s | K %d  E_ref %.3g / %.3g u (caps %.3g / %.3g)  E_plain %.3g / %.3g u (caps %g / %g)" % (
        (row.name, K) + f.e_ref + (cap_l2, cap_mx) + f.e_plain + ft.PLAIN_CAPS))
    assert f.e_ref[0] <= cap_l2 and f.e_ref[1] <= cap_mx, (row.name, f.e_ref, cap_l2, cap_mx)
    assert f.e_plain[0] <= ft.PLAIN_CAPS[0] and f.e_plain[1] <= ft.PLAIN_CAPS[1], (row.name, f.e_plain)
    # the impulses' plain overlap-save: within the same cap of the rounded taps (what the GPU test's impulse bar is built from)
    for p in ft.impulse_positions(row, f.n_in):
        xi = ft.impulse_input(row, f.x, p)
        e = ft.max_abs_err(row, ft.plain_ols(row, f.taps, xi, f.n_out), ft.impulse_truth(row, f.taps, p, f.n_out))
        assert e <= ft.PLAIN_CAPS[1] * ft.unit(row) * float(np.max(np.abs(f.taps))), (row.name, p, e / ft.unit(row))


@pytest.mark.parametrize("row", ft.DYN_ROWS, ids=[r.name for r in ft.DYN_ROWS])
def test_dynamic_range_inputs_and_their_figures(oracle, row):
    """the weak tone survives in the truth at its level, the strong one is gone: the input measures what it is meant to"""
    _skip_without_long_double(row)
    f = ft.dyn_figures(row)
    assert abs(float(np.sum(f.taps)) - row.L) < 1e-12 and f.n_out == (ft.DYN_ITERATIONS // row.M) * row.L
    level = float(np.sqrt(np.mean(np.abs(f.t).astype(np.float64) ** 2)))
    want = 1e-3 * (1 if ft.is_complex(row) else np.sqrt(0.5))
    assert 0.9 * want <= level <= 1.1 * want, (row.name, level)                   # the stop-band tone is 60 dB above it at the input
    print("FIRDYNCAP %s | E_ref %.3g u  E_plain %.3g u" % (row.name, f.e_ref, f.e_plain))
    # both references keep the weak tone: their errors are a fraction of u of ||h||_1 max|x|, 2^-10 of the weak tone or less
    assert 0 < f.e_ref <= 1 and 0 < f.e_plain <= 4, (row.name, f.e_ref, f.e_plain)


def test_every_row_names_a_plan_and_every_plan_has_a_row():
    from pothoscomms_amd import _lib
    for row in fp.PLANS + ft.DYN_ROWS:
        assert row.plan in _lib.FIR_PLANS and row.plan not in ("NONE", "CF32_OLS4096_GATED"), (row.name, row.plan)
        assert ft.time_domain(row) == (row.plan in ("CF32_DIRECT_TILE", "DOT2", "SLIDE", "GENERIC")), (row.name, row.plan)
    covered = set(r.plan for r in fp.PLANS)
    # the gated launch is reached through the rows of its ungated plan (test_plan_gated_call_contract calls every row gated)
    if any(r.plan == "CF32_OLS4096" and r.dtype == "complex_float32" and r.L == r.M == 1 and 1 < fp._K(r) <= 2049 for r in fp.PLANS):
        covered.add("CF32_OLS4096_GATED")
    assert covered == set(_lib.FIR_PLANS) - {"NONE"}, set(_lib.FIR_PLANS) - {"NONE"} - covered
    # every frequency-domain plan that a float stream reaches is also held to the truth
    float_plans = set(r.plan for r in ft.FLOAT_ROWS)
    assert float_plans == set(_lib.FIR_PLANS) - {"NONE", "CF32_OLS4096_GATED", "DOT2"}, float_plans
    assert len(set(r.name for r in fp.PLANS)) == len(fp.PLANS)


def test_plan_constants_follow_the_header():
    from pothoscomms_amd import _lib
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    declared = dict((name, int(v)) for name, v in re.findall(r"PCX_FIR_PLAN_(\w+)\s*=\s*(\d+)", src))
    assert declared == {name: i for i, name in enumerate(_lib.FIR_PLANS)}


def _degraded(row, t, rng, rms_u=None, one_sample=None):
    """the truth rounded to nothing but degraded on the host: + rms_u u (of the truth's rms) of noise, or one sample off by
    one_sample of the rms; returned in the wide type, as as_complex would hand a device output over"""
    a = np.abs(t).astype(np.float64)
    rms = float(np.sqrt(np.mean(a ** 2)))
    out = t.copy()
    if rms_u is not None:
        n = rng.normal(size=t.size) + (1j * rng.normal(size=t.size) if np.iscomplexobj(t) else 0)
        out = out + (n * (rms_u * ft.unit(row) * rms / (np.sqrt(2) if np.iscomplexobj(t) else 1))).astype(t.dtype)
    if one_sample is not None:
        out[t.size // 2] += one_sample * rms
    return out


@pytest.mark.parametrize("name", ["cf32 direct tile K=255 DIRECT", "f32 sliding K=1", "cf32 4096-sample K=255", "cf32 partitioned K=8193",
                                  "f32 real ols K=2049"])
def test_the_bars_can_fail(oracle, name):
    """a deliberately degraded output is over the bars.  Noise of 1.25 times the l2 bar fails l2 on any row; on a frequency-domain row
    that bar is 8 ... 12 u (plain_ols sits at 3 ... 6 u, the floor is 4 u), so 12.5 u rms of noise fails it -- 8 u rms would sit ON the
    bar of a row at the floor and under the others, so it is not what is asserted.  One sample off by 1e-4 of the rms (1678 u in
    float32) fails mx on any row.  An output that carries a quarter of the bar as noise passes both."""
    row = next(r for r in fp.PLANS if r.name == name)
    f = ft.noise_figures(row)
    bar_l2, bar_mx = ft.bars(row, f.e_ref, f.e_plain)
    rng = np.random.default_rng(1)
    clean = ft.l2_mx(row, f.t, f.t)
    assert clean == (0.0, 0.0)
    # twice the figure the bar is built from, as noise: "twice as bad on the same input" must fail, whatever the row
    noisy = ft.l2_mx(row, _degraded(row, f.t, rng, rms_u=1.25 * bar_l2), f.t)
    assert noisy[0] > bar_l2, (name, noisy, bar_l2)
    if not ft.time_domain(row):
        assert bar_l2 <= 2 * ft.PLAIN_CAPS[0] and 8 <= bar_l2 < 12.5                 # plain_ols sits at 3 ... 6 u: 12 u rms of noise fails it
        assert ft.l2_mx(row, _degraded(row, f.t, rng, rms_u=12.5), f.t)[0] > bar_l2
    spike = ft.l2_mx(row, _degraded(row, f.t, rng, one_sample=1e-4), f.t)
    assert spike[1] > bar_mx and 1e-4 / ft.unit(row) > bar_mx, (name, spike, bar_mx)
    # and an output as good as the figure itself passes
    fine = ft.l2_mx(row, _degraded(row, f.t, rng, rms_u=0.5 * bar_l2 / ft.FACTOR), f.t)
    assert fine[0] <= bar_l2 and fine[1] <= bar_mx, (name, fine, bar_l2, bar_mx)
