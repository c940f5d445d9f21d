"""Every plan of pcx_fir_process_dev through one table.

The planner (pothoscomms_amd/csrc/fir_plan.hpp) picks one of about twenty plans from the handle's settings, and the algorithm AUTO
stands for.  PLANS (tests/fir_plans.py) holds at least one row for each plan and each answer of AUTO, and a row on
either side of every bound that decides a plan.  Each row names the last_algo and the last_plan the call must report.  Three checks
run over the table:

1. guard bands and misaligned windows: input and output windows at element offsets 0, 1 and 3 inside poisoned buffers (NaN for
   floats, the type's extreme values for integers).  The outputs equal the oracle's work() on the window (bit for bit for integer
   and EXACT plans, otherwise within the bar of that plan's own parity test), no poison is written or read, and the three offsets
   give the same bits.  (Offsets count whole elements: a 16-byte element, complex float64 or complex int64, stays 16-byte aligned.)
2. reconfiguration: one handle per stream type walks through that type's rows, shuffled, three times, with the setters alone.
   Every call equals, bit for bit, a fresh handle given the same settings: no table of an earlier plan leaks into the next.
3. the gated call: only complex_float32 with M = L = 1, K <= 2049 on the overlap-save plan has a gate (include/pcx.h).  That
   plan must run gated and equal the plain call; every other row must return gated = 0 with nothing queued or written.
"""
import zlib

import numpy as np
import pytest

from tests.fir_plans import IDS, PLANS, _K, _configure, _make, _stream, _taps
from tests.util import TOL, bands_intact, diff_note, guarded, h2d

pytestmark = pytest.mark.gpu


def _setup():
    import torch

    from oracle import oracle as o
    return torch, o, {o.F32: torch.float32, o.F64: torch.float64, o.I64: torch.int64, o.I32: torch.int32, o.I16: torch.int16,
                      o.I8: torch.int8}


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
        assert f.last_plan == row.plan, (row.name, f.last_plan)
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
            got = (walker.process_dev(x, y, n_in, n_out), walker.last_algo, walker.last_plan, y)
            key = (row.name, q)
            if key not in fresh_out:
                ff = _make(dev, row, q)
                yf = torch.full_like(y, _fill(td, torch, False))
                fresh_out[key] = (ff.process_dev(x, yf, n_in, n_out), ff.last_algo, ff.last_plan, yf)
            want = fresh_out[key]
            assert got[:3] == want[:3], (row.name, q, got[:3], want[:3])
            # (the row's plan is the one under the process-wide Q-format reading: another reading gives other taps, and a row that sits
            # on the ||h_q|| bound of the integer overlap-save plans another plan)
            assert q is not None or got[2] == row.plan, (row.name, got[2])
            if not torch.equal(got[3].view(torch.uint8), want[3].view(torch.uint8)):
                g, w = got[3].cpu().numpy(), want[3].cpu().numpy()
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
        assert f.last_plan == "NONE", (row.name, f.last_plan)                  # nothing ran on this fresh handle
        assert bool((out == SENTINEL).all()), (row.name, "an ungated call wrote its output")
        return
    assert gated and (c, p) == (in_elems - (K - 1), out_cap) == (GATED_N, GATED_N), (row.name, gated, c, p)
    assert row.plan == "CF32_OLS4096" and f.last_plan == "CF32_OLS4096_GATED", (row.name, f.last_plan)
    refbuf.fill_(SENTINEL)
    assert f.process_dev(xin, refbuf, in_elems, out_cap) == (c, p)
    assert f.last_plan == row.plan, (row.name, f.last_plan)
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
