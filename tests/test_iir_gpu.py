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
CUTS = [1, 37, 100, 11, 251, 4096, 3500, 2004]       # 10000 samples: three tiles as one call, the last one partial
# orders 9 to 32 (the buckets NB = 16 and 32).  These cuts reach every one of the 32 carried history slots: several calls in a row
# shorter than the order (finish shifts the old history by 1, 1, 2, 5, 16, 7 and 31), calls of 31, 32 and 33, one that ends on the
# call's tile (4096) with a single sample behind it, and a last call of 1808
HIGH = M.high_order_set()
HIGH_SCAN = [k for k in HIGH if not k.startswith("unstable")]
HIGH_N = 10000
HIGH_CUTS = [1, 1, 2, 5, 16, 7, 31, 32, 33, 64, 4095 - 192, 4096, 1]
HIGH_CUTS.append(HIGH_N - sum(HIGH_CUTS))
_PLANS = {}


def model_bound(fname):
    if fname not in _PLANS:
        _PLANS[fname] = M.plan(HIGH[fname])
    assert _PLANS[fname][0] == "SCAN"
    return _PLANS[fname][1]


def scan_handle(h, fname):
    """h retuned to the filter fname of the high-order set; the handle's bound, which must be the model's and below 1e-10 (a
    handle that reported a large bound would pass anything)"""
    from pothoscomms_amd import _lib
    h.set_taps(HIGH[fname])
    plan, bound = h.plan()
    assert plan == _lib.IIR_SCAN and 0 < bound <= 1e-10, (fname, plan, bound)
    assert abs(bound - model_bound(fname)) <= 1e-6 * bound, (fname, bound, model_bound(fname))
    return bound


def xmax(x):
    return float(np.max(np.abs(x.astype(np.float64))))


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


# ---- orders 9 to 32
@pytest.mark.parametrize("dtype", DTYPES)
def test_high_order_buckets_within_the_bound_cut_whole_and_device(dev, dtype):
    """every type on NB = 16 and 32: one handle retuned 16 -> 16 -> 32 -> 32 -> 16 -> 32, each stream in HIGH_CUTS, whole, and
    through process_dev"""
    import torch
    name, cplx = M.split(dtype)
    assert sum(HIGH_CUTS) == HIGH_N and HIGH_CUTS[-1] > 0
    h = dev.IIRFilter(dtype)
    for fname in ("spread9", "spread16", "spread17", "spread32", "comb16", "comb32"):
        bound = scan_handle(h, fname)
        for kind in ("noise", "full"):
            x = stream(dtype, HIGH_N, kind, zlib.crc32(("%s/%s/%s" % (dtype, fname, kind)).encode()))
            yd, _ = M.run(x, HIGH[fname], name)
            tol = bound * xmax(x)
            h.reset()
            cut = feed(h, x, HIGH_CUTS)
            assert within(cut, yd, tol, name), (dtype, fname, kind, "cut")
            h.reset()
            whole = h.process(x)
            assert within(whole, yd, tol, name), (dtype, fname, kind, "whole")
            h.reset()
            yt = torch.empty_like(_torch_of(x))
            h.process_dev(_torch_of(x), yt, HIGH_N)
            assert np.array_equal(yt.cpu().numpy(), whole, equal_nan=name.startswith("float")), (dtype, fname, kind, "dev")


@pytest.mark.parametrize("dtype", ["float64", "complex_int16"])
def test_every_high_order_scan_filter_in_cuts(dev, dtype):
    """the orders between the buckets' ends as well (12, 24, 31) and every comb"""
    name, cplx = M.split(dtype)
    h = dev.IIRFilter(dtype)
    for fname in HIGH_SCAN:
        bound = scan_handle(h, fname)
        x = stream(dtype, HIGH_N, "noise", zlib.crc32(fname.encode()))
        yd, _ = M.run(x, HIGH[fname], name)
        assert within(feed(h, x, HIGH_CUTS), yd, bound * xmax(x), name), (dtype, fname)


def test_comb32_impulse_is_exactly_half_to_the_j_every_32_samples_on_scan(dev):
    """a = 1 - 0.5 z^-32, b = 1: every entry of every table is 0 or a power of two, every sum has one term that is not zero"""
    from pothoscomms_amd import _lib
    taps = [1.0] + [0.0] * 32 + [1.0] + [0.0] * 31 + [-0.5]
    h = dev.IIRFilter("float64", taps)
    assert h.plan()[0] == _lib.IIR_SCAN
    x = np.zeros(9000)
    x[0] = 1.0
    want = np.zeros(9000)
    want[::32] = np.ldexp(1.0, -np.arange(len(want[::32])))
    assert np.array_equal(h.process(x), want)
    h.reset()
    assert np.array_equal(feed(h, x, [1, 31, 1, 4063, 4904]), want)


@pytest.mark.parametrize("fname", ["spread17", "comb32"])
@pytest.mark.parametrize("dtype", ["float64", "complex_int16"])
def test_carry_second_level_against_the_model(dev, dtype, fname):
    """66 tiles in one call: the carry kernel's scan over runs of 64 tiles hands thread 1 its incoming state; and the same stream cut
    three samples in front of the 64th tile's end"""
    name, cplx = M.split(dtype)
    n = 65 * 4096 + 7
    h = dev.IIRFilter(dtype)
    bound = scan_handle(h, fname)
    x = stream(dtype, n, "noise", zlib.crc32(("carry/%s/%s" % (dtype, fname)).encode()))
    yd, _ = M.run(x, HIGH[fname], name)
    tol = bound * xmax(x)
    assert within(h.process(x), yd, tol, name), "whole"
    h.reset()
    assert within(feed(h, x, [64 * 4096 - 3, 4096 + 10]), yd, tol, name), "cut"


@pytest.mark.parametrize("fname", ["spread32", "comb32"])
@pytest.mark.parametrize("dtype", ["complex_float32", "float64"])
def test_high_order_1mi_samples_by_the_residual_on_the_device(dev, dtype, fname):
    import torch
    name, cplx = M.split(dtype)
    n = 1 << 20
    h = dev.IIRFilter(dtype)
    bound = scan_handle(h, fname)
    g = torch.Generator(device="cuda:0").manual_seed(14)
    x = torch.rand((n, 2) if cplx else (n,), device="cuda:0", generator=g, dtype=getattr(torch, name)) * 2 - 1
    y = torch.empty_like(x)
    h.process_dev(x, y, n)
    assert M.residual_check(x.to(torch.float64), y.to(torch.float64), HIGH[fname], name, bound) == -1


@pytest.mark.parametrize("dtype", ["float64", "complex_float32", "int8", "int64", "complex_int16"])
def test_high_order_unstable_filters_are_serial_and_bit_exact(dev, dtype):
    """the SERIAL loop and its rings at orders 3 to 32, the history carried over calls shorter than, equal to and longer than the
    order and the ring"""
    from pothoscomms_amd import _lib
    name, cplx = M.split(dtype)
    cuts = [1, 2, 5, 31, 32, 33, 63, 64, 65]
    cuts.append(3000 - sum(cuts))
    h = dev.IIRFilter(dtype)
    for fname in HIGH:
        if not fname.startswith("unstable"):
            continue
        h.set_taps(HIGH[fname])
        assert h.plan() == (_lib.IIR_SERIAL, 0.0), fname
        x = stream(dtype, 3000, "noise", zlib.crc32(fname.encode()))
        _, want = M.run(x, HIGH[fname], name)
        assert same(feed(h, x, cuts), want), (dtype, fname)


@pytest.mark.parametrize("dtype", ["int8", "complex_float64"])
def test_high_order_odd_lengths_leave_the_guard_bands_alone(dev, dtype):
    import torch
    name, cplx = M.split(dtype)
    guard = 4096
    h = dev.IIRFilter(dtype)
    bound = scan_handle(h, "spread32")
    for n in (1, 31, 4095, 4096, 4097):
        x = stream(dtype, n, "noise", 40 + n)
        yd, _ = M.run(x, HIGH["spread32"], name)
        for off in (1, 3):
            total = guard + off + n + guard
            raw = torch.full((total * x.itemsize * (2 if cplx else 1),), 0xA5, dtype=torch.uint8, device="cuda:0")
            buf = raw.view(getattr(torch, name)).reshape((total, 2) if cplx else (total,))
            h.reset()
            h.process_dev(_torch_of(x), buf[guard + off:guard + off + n], n)
            got = buf.cpu().numpy()
            lo, hi = got[:guard + off], got[guard + off + n:]
            assert np.all(lo.view(np.uint8) == 0xA5) and np.all(hi.view(np.uint8) == 0xA5), (dtype, n, off)
            assert within(got[guard + off:guard + off + n], yd, bound * xmax(x), name), (dtype, n, off)


def test_block_with_the_66_taps_of_order_32(dev):
    from pothoscomms_amd import blocks as B
    taps = HIGH["spread32"]
    assert len(taps) == 66
    x = stream("complex_float32", 10000, "noise", 31)
    blk = B.make("/comms/iir_filter", "complex_float32", module="iir")
    blk.call("setTaps", taps)
    assert np.array_equal(blk.call("getTaps"), taps)
    blk.activate()
    y, consumed, produced, _, _ = blk.work(x, 10000)
    assert consumed == produced == 10000
    assert np.array_equal(y[:produced], dev.IIRFilter("complex_float32", taps).process(x))


def test_overlapping_buffers_are_refused_and_the_handle_stays_good(dev):
    """the apply kernel reads a tile's halo and the finish kernel the last inputs after outputs have been written: any overlap of
    the n input with the n output elements is refused before the device is touched, out == in included"""
    import torch
    from pothoscomms_amd import _lib
    taps = HIGH["spread32"]
    x = stream("complex_float32", 10000, "noise", 32)
    f = dev.IIRFilter("complex_float32", taps)
    fresh = [f.process(x[:100]), f.process(x[100:])]
    h = dev.IIRFilter("complex_float32", taps)
    assert np.array_equal(h.process(x[:100]), fresh[0])       # a history that a refused call must leave alone
    xd = _torch_of(x)
    for a, b in ((xd, xd), (xd[:1000], xd[1:1001]), (xd[8:1008], xd[:1000]), (xd[:5000], xd[4999:9999])):
        with pytest.raises(_lib.InvalidArgument, match="overlaps"):
            h.process_dev(a, b, a.shape[0])
    xh = x.copy()
    for a, b in ((xh, xh), (xh[:1000], xh[1:1001]), (xh[999:1999], xh[:1000])):
        with pytest.raises(_lib.InvalidArgument, match="overlaps"):
            h.process(a, out=b)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(xh, x)
    assert np.array_equal(h.process(x[100:]), fresh[1])
    # buffers that touch without overlapping are accepted
    f.reset()
    want = np.concatenate([f.process(x[:5000]), f.process(x[5000:])])
    h.reset()
    yd = torch.empty_like(xd)
    h.process_dev(xd[:5000], yd[:5000], 5000)
    h.process_dev(xd[5000:], xd[:5000], 5000)
    assert np.array_equal(torch.cat([yd[:5000], xd[:5000]]).cpu().numpy(), want)
