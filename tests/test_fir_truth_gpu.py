"""Every float FIR plan against a wider truth (tests/fir_truth.py), on the inputs of the shared table (tests/fir_plans.py).

The parity tests hold the plans to the oracle's float FIR at 1e-5 of max|ref| (168 u in float32; 1e-13, 900 u, in double).  The oracle
is the reference's sequential sum in the device's own precision and sits 0.3 sqrt(K) u from the truth; a plain overlap-save sits at
3 ... 6 u whatever K.  So those bars are 10 ... 80 times what a sound plan does.  Here every row asserts the plan it ran and then

(a) noise: l2 and mx of the row's own call against the truth under 2 max(E, floor): E is the oracle's figure for a time-domain plan
    and the plain overlap-save's (plain_ols) for a frequency-domain plan, on the same input; floors 4 u and 16 u;
(b) impulses: a 1 at iteration 0, 1, 4095, 4096 (those inside the stream: a 64-fold interpolator's is 777 iterations long), one call
    each.  The true output is the rounded taps laid out by the polyphase rule.  A time-domain plan returns them exactly; a
    frequency-domain plan within 2 max(E_plain, 4 u) max|h|, E_plain plain_ols's worst over the same inputs.  A tap table one
    entry short, or an overlap off by one at a block seam, shows at full size;
(c) dynamic range: a unit tone in the stop band over one 60 dB weaker in the pass band through a Blackman-windowed sinc, one row per
    frequency-domain kernel family: max|got - t| / (||h||_1 max|x|) under 2 max(E_ref, E_plain), no floor.

No bar comes from the device's output.  Every case prints its figures (FIRACC lines, in u) before it asserts.  PLAIN_BAR_WAIVED lists
the rows, four at the most, that meet 2 max(E_ref, E_plain, floor) but not the plain overlap-save's bar, each with its cause.
"""
import numpy as np
import pytest

from tests import fir_plans as fp
from tests import fir_truth as ft
from tests.util import h2d

pytestmark = pytest.mark.gpu

# row name -> cause (file and line, DESIGN.md "FIR accuracy"); such a row is held to 2 max(E_ref, E_plain, floor)
PLAIN_BAR_WAIVED = {}
assert len(PLAIN_BAR_WAIVED) <= 4

IDS = [r.name for r in ft.FLOAT_ROWS]


def _skip_without_long_double(row):
    if ft.needs_long_double(row) and not ft.LD_IS_EXTENDED:
        pytest.skip("numpy.longdouble is no wider than float64 here (eps %.3g): there is no truth for a float64 stream" % ft.LD_EPS)


def _run(dev, f, row, x, n_in, n_out):
    """one device call on host input x; the output as numpy, after the plan has been checked"""
    import torch
    d = torch.device("cuda", 0)
    td = torch.float32 if ft.np_dtype(row) == np.float32 else torch.float64
    y = torch.full((n_out, 2) if ft.is_complex(row) else (n_out,), float("nan"), dtype=td, device=d)
    c, p = f.process_dev(h2d(np.array(x), d), y, n_in, n_out)          # (a copy: the shared input is read-only)
    torch.cuda.synchronize()
    assert p == n_out, (row.name, c, p, n_out)
    assert f.last_plan == row.plan, (row.name, f.last_plan, row.plan)
    got = y.cpu().numpy()
    assert not np.isnan(got).any(), (row.name, "an output left unwritten")
    return got


@pytest.mark.parametrize("row", ft.FLOAT_ROWS, ids=IDS)
def test_noise_against_the_truth(oracle, dev, row):
    _skip_without_long_double(row)
    fig = ft.noise_figures(row)
    got = _run(dev, fp._make(dev, row), row, fig.x, fig.n_in, fig.n_out)
    l2, mx = ft.l2_mx(row, got, fig.t)
    bar_l2, bar_mx = ft.bars(row, fig.e_ref, fig.e_plain, waived=row.name in PLAIN_BAR_WAIVED)
    print("FIRACC noise l2 | %s | %s | err %.3g | E_ref %.3g | E_plain %.3g | bar %.3g | ratio %.2f" % (
        row.name, row.plan, l2, fig.e_ref[0], fig.e_plain[0], bar_l2, l2 / bar_l2))
    print("FIRACC noise mx | %s | %s | err %.3g | E_ref %.3g | E_plain %.3g | bar %.3g | ratio %.2f" % (
        row.name, row.plan, mx, fig.e_ref[1], fig.e_plain[1], bar_mx, mx / bar_mx))
    assert l2 <= bar_l2 and mx <= bar_mx, (row.name, row.plan, "l2 %.3g u of %.3g, mx %.3g u of %.3g" % (l2, bar_l2, mx, bar_mx))


@pytest.mark.parametrize("row", ft.FLOAT_ROWS, ids=IDS)
def test_impulses_return_the_taps(oracle, dev, row):
    _skip_without_long_double(row)
    fig = ft.noise_figures(row)              # the lengths of the row's own stream
    u, hmax = ft.unit(row), float(np.max(np.abs(ft.rounded_taps(row, fig.taps)).astype(np.float64)))
    f = fp._make(dev, row)
    ps = ft.impulse_positions(row, fig.n_in)
    assert ps[:2] == [0, 1]
    errs, e_plain = [], 0.0
    for p in ps:
        xi = ft.impulse_input(row, fig.x, p)
        t = ft.impulse_truth(row, fig.taps, p, fig.n_out)
        got = _run(dev, f, row, xi, fig.n_in, fig.n_out)
        if ft.time_domain(row):
            real_t, cplx_t = ft._wide(row)
            same = np.array_equal(ft.as_complex(got, real_t, cplx_t), t)          # as values: -0.0 equals 0.0
            print("FIRACC impulse | %s | %s | p %d | exact %s" % (row.name, row.plan, p, same))
            assert same, (row.name, row.plan, p, ft.max_abs_err(row, got, t) / u / hmax)
            continue
        errs.append(ft.max_abs_err(row, got, t) / u / hmax)
        e_plain = max(e_plain, ft.max_abs_err(row, ft.plain_ols(row, fig.taps, xi, fig.n_out), t) / u / hmax)
    if errs:
        bar = ft.FACTOR * max(e_plain, ft.FLOOR_L2)
        print("FIRACC impulse | %s | %s | err %s | E_plain %.3g | bar %.3g | ratio %.2f" % (
            row.name, row.plan, " ".join("%.3g" % e for e in errs), e_plain, bar, max(errs) / bar))
        assert max(errs) <= bar, (row.name, row.plan, errs, bar)


@pytest.mark.parametrize("row", ft.DYN_ROWS, ids=[r.name for r in ft.DYN_ROWS])
def test_dynamic_range(oracle, dev, row):
    _skip_without_long_double(row)
    fig = ft.dyn_figures(row)
    f = dev.FirFilter(row.dtype, row.taps)
    f.set_taps(fig.taps); f.set_decimation(row.M); f.set_interpolation(row.L)
    got = _run(dev, f, row, fig.x, fig.n_in, fig.n_out)
    err = ft.dyn_err(row, got, fig.t, fig.taps, fig.x)
    bar = ft.FACTOR * max(fig.e_ref, fig.e_plain)
    print("FIRACC dynamic | %s | %s | err %.3g | E_ref %.3g | E_plain %.3g | bar %.3g | ratio %.2f" % (
        row.name, row.plan, err, fig.e_ref, fig.e_plain, bar, err / bar))
    assert err <= bar, (row.name, row.plan, err, bar)


def test_waived_rows_are_rows_of_the_table():
    assert len(PLAIN_BAR_WAIVED) <= 4
    for name in PLAIN_BAR_WAIVED:
        row = next(r for r in ft.FLOAT_ROWS if r.name == name)
        assert not ft.time_domain(row), name
