"""GPU suite of /comms/iir_filter (pcx_iir_*, device.IIRFilter, the block in libpcx_iir_blocks.so).

SCAN outputs are held to the handle's bound against the sequential model (tests/iir_model.py): before narrowing within bound * max|x|
of the model's double value, so after it between the narrowings of the two ends of that interval.  SERIAL outputs are held to the
model bit for bit.  Long streams are checked by the residual of the recurrence, on the device."""
import zlib

import numpy as np
import pytest

import iir_model as M

pytestmark = pytest.mark.gpu

TYPES = list(M.SCALARS)
DTYPES = TYPES + ["complex_" + t for t in TYPES]
CUTS = [1, 37, 100, 11, 251, 4096, 3500, 2004]       # 10000 samples, four tiles


def _torch_of(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def stream(dtype, n, kind, seed):
    name, cplx = M.split(dtype)
    t = M.SCALARS[name]
    rng = np.random.default_rng(seed)
    shape = (n, 2) if cplx else (n,)
    if name.startswith("float"):
        scale = {"noise": 1.0, "full": 1e6, "extreme": 1e30 if name == "float32" else 1e300}[kind]
        return (rng.uniform(-1, 1, shape) * scale).astype(t)
    info = np.iinfo(t)
    if kind == "noise":
        return rng.integers(info.min // 8, info.max // 8, shape, endpoint=True, dtype=t)
    if kind == "full":
        return rng.integers(info.min, info.max, shape, endpoint=True, dtype=t)
    x = np.where(np.arange(n) % 2 == 0, info.max, info.min).astype(t)     # full-scale square wave at Nyquist, then runs at the rails
    x[n // 2:] = np.where((np.arange(n - n // 2) // 700) % 2 == 0, info.max, info.min)
    return np.stack([x, x[::-1]], 1).copy() if cplx else x


def within(got, yd, tol, name):
    """got (narrowed device outputs) between the narrowings of yd -+ tol; NaN where the model is NaN (0 for integers)"""
    lo, hi = M.narrow(yd - tol, name), M.narrow(yd + tol, name)
    nan = np.isnan(yd)
    ok = (got >= lo) & (got <= hi)
    if name.startswith("float"):
        ok = np.where(nan, np.isnan(got), ok)
    else:
        ok = np.where(nan, got == 0, ok)
    return bool(np.all(ok))


def same(got, want):
    """bit for bit, any NaN for a NaN (the default NaN's sign differs between x86-64 and the GPU)"""
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint8), want[~nan].view(np.uint8)))


def feed(h, x, cuts):
    outs, pos = [], 0
    for c in cuts:
        outs.append(h.process(x[pos:pos + c]))
        pos += c
    assert pos == x.shape[0]
    return np.concatenate(outs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_named_set_scan_within_the_bound_cut_whole_and_device(dev, dtype):
    import torch
    from pothoscomms_amd import _lib
    name, cplx = M.split(dtype)
    n = sum(CUTS)
    for fname, taps in M.named_set().items():
        h = dev.IIRFilter(dtype, taps)
        plan, bound = h.plan()
        assert plan == _lib.IIR_SCAN and 0 < bound <= 1e-10, (fname, plan, bound)
        assert abs(bound - M.plan(taps)[1]) <= 1e-6 * bound
        for kind in ("noise", "full", "extreme"):
            x = stream(dtype, n, kind, zlib.crc32(("%s/%s/%s" % (dtype, fname, kind)).encode()))
            yd, _ = M.run(x, taps, name)
            tol = bound * float(np.max(np.abs(x.astype(np.float64))))
            h.reset()
            cut = feed(h, x, CUTS)
            assert within(cut, yd, tol, name), (dtype, fname, kind, "cut")
            h.reset()
            whole = h.process(x)
            assert within(whole, yd, tol, name), (dtype, fname, kind, "whole")
            h.reset()
            yt = torch.empty_like(_torch_of(x))
            h.process_dev(_torch_of(x), yt, n)
            assert np.array_equal(yt.cpu().numpy(), whole, equal_nan=name.startswith("float")), (dtype, fname, kind, "dev")


@pytest.mark.parametrize("dtype", ["complex_float64", "float32", "int16"])
def test_stress_filter_scan_within_its_own_bound(dev, dtype):
    from pothoscomms_amd import _lib
    name, _ = M.split(dtype)
    taps = M.taps_of(M.butter(8, 0.1))
    h = dev.IIRFilter(dtype, taps)
    plan, bound = h.plan()
    assert plan == _lib.IIR_SCAN and 0 < bound < 1e-2
    x = stream(dtype, 20000, "noise", 21)
    yd, _ = M.run(x, taps, name)
    assert within(h.process(x), yd, bound * float(np.max(np.abs(x.astype(np.float64)))), name)


def test_first_order_impulse_is_exactly_half_to_the_n_on_scan(dev):
    from pothoscomms_amd import _lib
    h = dev.IIRFilter("float64", [1.0, 0.0, 1.0, -0.5])
    assert h.plan()[0] == _lib.IIR_SCAN
    x = np.zeros(9000)
    x[0] = 1.0
    want = np.ldexp(1.0, -np.arange(9000))          # 2^-n, subnormals and the zeros past them included
    assert np.array_equal(h.process(x), want)


@pytest.mark.parametrize("dtype", ["float64", "complex_float32", "int8", "int64", "complex_int16"])
def test_unstable_and_integrator_filters_are_serial_and_bit_exact(dev, dtype):
    from pothoscomms_amd import _lib
    name, cplx = M.split(dtype)
    for taps in ([1.0, 0.0, 1.0, -1.01], [1.0, 0.0, 1.0, -1.0], [1.0, 0.0, 0.0, 1.0, -2.5, 1.0]):
        h = dev.IIRFilter(dtype, taps)
        assert h.plan() == (_lib.IIR_SERIAL, 0.0), taps
        x = stream(dtype, 3000, "noise", 5)
        if name.startswith("float"):
            x[1500] = np.inf
        _, want = M.run(x, taps, name)
        got = feed(h, x, [1, 999, 2000])
        assert same(got, want), (dtype, taps)


def test_int_saturation_and_nan_to_zero_on_serial(dev):
    taps = [1.0, 0.0, 0.0, 1.0, -2.5, 1.0]              # poles 2 and 0.5: grows to inf, then inf - inf
    for dtype in ("int8", "int64"):
        h = dev.IIRFilter(dtype, taps)
        x = stream(dtype, 2000, "noise", 6)
        yd, want = M.run(x, taps, dtype)
        got = h.process(x)
        assert np.array_equal(got, want)
        info = np.iinfo(M.SCALARS[dtype])
        assert np.isnan(yd).any() and np.all(got[np.isnan(yd)] == 0)
        assert np.any(got == info.max) or np.any(got == info.min)


def test_gain_two_on_int8_saturates(dev):
    from pothoscomms_amd import _lib
    h = dev.IIRFilter("int8", [2.0, 1.0])
    assert h.plan()[0] == _lib.IIR_SCAN
    x = np.arange(-128, 128, dtype=np.int8)
    assert np.array_equal(h.process(x), np.clip(2 * x.astype(np.int32), -128, 127).astype(np.int8))


def _tone(n, f, fs):
    return np.exp(2j * np.pi * f / fs * np.arange(n))


def test_reference_test_through_the_block(dev):
    """TestIIRFilter.cpp:11-60: a complex_float64 tone through the block, taps from a 4th-order Butterworth at 0.1 set at runtime"""
    from pothoscomms_amd import blocks as B
    b, a = M.butter(4, 0.2)
    taps = M.taps_of((b, a))
    for f, check in ((30e3, "pass"), (300e3, "stop")):
        x = _tone(4096, f, 1e6)
        blk = B.make("/comms/iir_filter", "complex_float64", module="iir")
        blk.call("setWaitTaps", True)
        assert blk.call("getWaitTaps")
        blk.activate()
        pairs = x.view(np.float64).reshape(-1, 2).copy()
        _, consumed, produced, _, _ = blk.work(pairs, 4096)
        assert consumed == 0 and produced == 0             # armed: nothing before the taps
        blk.call("setTaps", taps)
        y, consumed, produced, _, _ = blk.work(pairs, 4096)
        assert consumed == produced == 4096
        yc = y[:produced, 0] + 1j * y[:produced, 1]
        w = 2 * np.pi * f / 1e6
        H = abs(np.polyval(b[::-1], np.exp(-1j * w)) / np.polyval(a[::-1], np.exp(-1j * w)))
        if check == "pass":
            assert np.sqrt(np.mean(np.abs(yc) ** 2)) > 0.1
            assert np.all(np.abs(np.abs(yc[500:]) - H) <= 0.01 * H)
        else:
            assert np.max(np.abs(yc[500:])) < 0.01


def test_block_activate_resets_and_settaps_resets(dev):
    from pothoscomms_amd import blocks as B
    x = stream("float32", 5000, "noise", 8)
    blk = B.make("/comms/iir_filter", "float32", module="iir")
    assert np.allclose(blk.call("getTaps"), M.DEFAULT_TAPS)
    blk.activate()
    y1, _, p1, _, _ = blk.work(x, 5000)
    blk.deactivate()
    blk.activate()
    y2, _, p2, _, _ = blk.work(x, 5000)
    assert p1 == p2 == 5000 and np.array_equal(y1[:p1], y2[:p2])
    with pytest.raises(Exception):
        blk.call("setTaps", [1.0, 2.0, 3.0])


def test_nan_mid_stream(dev):
    x = stream("float64", 20000, "noise", 9)
    x[9000] = np.nan
    h = dev.IIRFilter("float64")
    y = h.process(x)
    assert np.all(np.isfinite(y[:9000])) and not np.any(np.isfinite(y[9000:]))


def test_set_taps_mid_stream_resets_and_changes_order(dev):
    x = stream("complex_float32", 30000, "noise", 10)
    h = dev.IIRFilter("complex_float32")
    h.process(x[:7000])
    for taps in (M.named_set()["butter6_0.2"], M.named_set()["butter2_0.01"], M.taps_of(M.butter(8, 0.1))):
        h.set_taps(taps)
        assert np.allclose(h.taps(), taps)
        got = h.process(x[7000:])
        fresh = dev.IIRFilter("complex_float32", taps).process(x[7000:])
        assert np.array_equal(got, fresh)


def test_graph_capture_replays_bit_equal(dev):
    import torch
    n = 1 << 20
    x = stream("complex_float32", 3 * n, "noise", 12)
    ref = dev.IIRFilter("complex_float32", M.named_set()["butter4_0.1"])
    want = np.concatenate([ref.process(x[k * n:(k + 1) * n]) for k in range(3)])
    h = dev.IIRFilter("complex_float32", M.named_set()["butter4_0.1"])
    xd = _torch_of(x)
    yd = torch.empty_like(xd)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        h.process_dev(xd[:n], yd[:n], n, stream=s)      # tables uploaded, stream bound
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        h.reset()
        for k in range(3):
            h.process_dev(xd[k * n:(k + 1) * n], yd[k * n:(k + 1) * n], n, stream=s)
    for _ in range(2):
        yd.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", ["complex_float32", "float32", "complex_int16"])
def test_64mi_samples_by_the_residual_on_the_device(dev, dtype):
    import torch
    name, cplx = M.split(dtype)
    n = 64 << 20
    taps = M.named_set()["butter4_0.1"]
    h = dev.IIRFilter(dtype, taps)
    _, bound = h.plan()
    g = torch.Generator(device="cuda:0").manual_seed(4)
    shape = (n, 2) if cplx else (n,)
    if name == "float32":
        x = torch.rand(shape, device="cuda:0", generator=g, dtype=torch.float32) * 2 - 1
    else:
        x = torch.randint(-4096, 4096, shape, device="cuda:0", generator=g, dtype=torch.int16)
    y = torch.empty_like(x)
    h.process_dev(x, y, n)
    assert M.residual_check(x.to(torch.float64), y.to(torch.float64), taps, name, bound) == -1


def test_beyond_2_31_elements(dev):
    import torch
    n = (1 << 31) + 12345
    free, _ = torch.cuda.mem_get_info()
    if free < n * 4 + (3 << 30):
        pytest.skip("needs %d bytes of device memory" % (n * 4 + (3 << 30)))
    taps = M.DEFAULT_TAPS
    x = torch.randint(-16, 16, (n,), dtype=torch.int8, device="cuda:0")
    y = torch.empty_like(x)
    h = dev.IIRFilter("int8", taps)
    _, bound = h.plan()
    h.process_dev(x, y, n)
    torch.cuda.synchronize()
    # the residual in pieces that reach back by the order: each piece's first two residuals lack their history and are skipped
    step = 1 << 27
    for a0 in range(0, n, step):
        lo, b0 = max(0, a0 - 2), min(n, a0 + step)
        xs, ys = x[lo:b0].to(torch.float64), y[lo:b0].to(torch.float64)
        assert M.residual_check(xs, ys, taps, "int8", bound, xmax=16.0, skip=a0 - lo) == -1, a0
        del xs, ys
