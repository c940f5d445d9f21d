"""GPU suite of /comms/dc_removal (pcx_dcremoval_*, device.DCRemoval, the block in libpcx_filter_blocks.so).

Integer types are held bit for bit to the reference's recorded outputs (tests/golden/dcremoval.npz) and, on longer streams, to the
numpy restatement that equals them (tests/dcr_model.py, tests/test_dcremoval_cpu.py).  Float types are held to the exact-arithmetic
restatement (1e-6 of max|x| for float32, 1e-13 for float64) and, loosely, to the reference's own drifting outputs."""
import numpy as np
import pytest

import dcr_model as M

pytestmark = pytest.mark.gpu

DTYPES = [t for t in M.SCALARS] + ["complex_" + t for t in M.SCALARS]
TOL = {"float32": 1e-6, "float64": 1e-13}


def np_type(dtype):
    return M.SCALARS[M.split(dtype)[0]]


def rand_stream(dtype, n, seed, amp=None):
    name, cplx = M.split(dtype)
    rng = np.random.default_rng(seed)
    shape = (n, 2) if cplx else (n,)
    if name.startswith("float"):
        return rng.uniform(-1.0, 1.0, shape).astype(M.SCALARS[name])
    info = np.iinfo(M.SCALARS[name])
    lo, hi = (info.min, info.max) if amp is None else (-amp, amp)
    return rng.integers(lo, hi, shape, endpoint=True, dtype=M.SCALARS[name])


def assert_matches(got, x, dtype, D, C, what=""):
    want = M.restate(x, dtype, D, C)
    name, _ = M.split(dtype)
    if name in TOL:
        err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) / max(float(np.max(np.abs(x))), 1e-300)
        assert err <= TOL[name], (dtype, D, C, what, err)
    else:
        bad = np.nonzero(np.any((got != want).reshape(got.shape[0], -1), axis=1))[0]
        assert bad.size == 0, (dtype, D, C, what, bad[:5], got[bad[:3]], want[bad[:3]])


def golden_cases():
    z = np.load(__file__.replace("test_dcremoval_gpu.py", "golden/dcremoval.npz"))
    for k in z.files:
        if k.startswith("out/"):
            _, dtype, pattern, D, C = k.split("/")
            ref = z[k]
            yield dtype, pattern, int(D), int(C), z["in/%s/%s" % (dtype, pattern)][:ref.shape[0]], ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_fixture_case(dev, dtype):
    n = 0
    for dt, pattern, D, C, x, ref in golden_cases():
        if dt != dtype:
            continue
        got = dev.DCRemoval(dtype, D, C).process(x)
        name, _ = M.split(dtype)
        if name in TOL:
            assert_matches(got, x, dtype, D, C, pattern)
            err = float(np.max(np.abs(got.astype(np.float64) - ref))) / max(float(np.max(np.abs(x))), 1e-30)
            assert err <= 1e-3, (dtype, pattern, D, C, err)
        else:
            assert np.array_equal(got, ref), (dtype, pattern, D, C)
        n += 1
    assert n == (45 if dtype == "complex_int8" else 54)


def test_refused_configurations_leave_out_untouched(dev, pcx):
    for dtype, D in (("complex_int8", 512), ("complex_int8", 256), ("int8", 65536)):
        h = dev.DCRemoval(dtype, D, 2)
        x = rand_stream(dtype, 1000, 3)
        out = np.full_like(x, 77)
        with pytest.raises(pcx._lib.InvalidArgument, match="divides by zero"):
            h.process(x, out=out)
        assert np.all(out == 77)
    # the default size of complex_int8 is such a configuration: the handle is made, the call is refused
    h = dev.DCRemoval("complex_int8")
    assert h.sizes() == (512, 2)
    with pytest.raises(pcx._lib.InvalidArgument):
        h.process(rand_stream("complex_int8", 10, 1))


@pytest.mark.parametrize("dtype,D,C", [("int64", 64, 2), ("complex_int16", 64, 2), ("complex_float32", 512, 2), ("int32", 7, 3),
                                       ("int8", 64, 3), ("complex_int8", 100, 2), ("float64", 3000, 1), ("int16", 1500, 2)])
def test_a_stream_cut_into_calls_equals_one_call(dev, dtype, D, C):
    sizes = [1, D - 1, D, D + 1, 4099, 1, 300001, D + 1, 5]
    sizes = [s for s in sizes if s > 0]
    x = rand_stream(dtype, sum(sizes), 11)
    one = dev.DCRemoval(dtype, D, C).process(x)
    h = dev.DCRemoval(dtype, D, C)
    parts, o = [], 0
    for s in sizes:
        parts.append(h.process(x[o:o + s]))
        o += s
    cut = np.concatenate(parts)
    if M.split(dtype)[0] in TOL:
        assert np.max(np.abs(cut.astype(np.float64) - one)) <= TOL[M.split(dtype)[0]] * np.max(np.abs(x))
    else:
        assert np.array_equal(cut, one)
    assert_matches(one, x, dtype, D, C)


@pytest.mark.parametrize("dtype,D,C", [("complex_int16", 100, 3), ("float32", 100, 3), ("int8", 100, 3),
                                       # staged state whose byte size is no multiple of 4: every byte of it is reset
                                       ("complex_int8", 2049, 1), ("complex_int8", 683, 3), ("int8", 4097, 1)])
def test_set_sizes_or_reset_mid_stream_is_a_fresh_handle(dev, dtype, D, C):
    x = rand_stream(dtype, 20000, 5)
    h = dev.DCRemoval(dtype, 32, 2)
    h.process(x[:7000])
    h.set_sizes(D, C)
    assert np.array_equal(h.process(x[7000:]), dev.DCRemoval(dtype, D, C).process(x[7000:]))
    h.process(x[:12345])
    h.reset()
    got = h.process(x)
    assert np.array_equal(got, dev.DCRemoval(dtype, D, C).process(x))
    assert_matches(got, x, dtype, D, C)


@pytest.mark.parametrize("D,C", [(1, 1), (2, 2), (3, 3), (7, 2), (512, 2), (3000, 1)])
def test_float64_with_a_dc_offset(dev, D, C):
    """the use case: a large DC level under a small signal -- exact to 1e-13 of max|x| (fused up to a 2048-sample halo, staged
    beyond)"""
    rng = np.random.default_rng(D * 10 + C)
    for cplx in (False, True):
        shape = (60000, 2) if cplx else (60000,)
        x = (1000.0 + rng.uniform(-1.0, 1.0, shape)).astype(np.float64)
        dtype = "complex_float64" if cplx else "float64"
        assert_matches(dev.DCRemoval(dtype, D, C).process(x), x, dtype, D, C)
    x = (rng.uniform(-1.0, 1.0, (60000, 2)) + 300.0).astype(np.float32)
    assert_matches(dev.DCRemoval("complex_float32", D, C).process(x), x, "complex_float32", D, C)


def test_a_failed_set_sizes_leaves_no_usable_handle(dev, pcx):
    """sizes the device cannot hold (2^30 x 1024 complex_float64 samples of history): set_sizes fails, the handle refuses calls
    until sizes are set again, and then runs as a fresh one"""
    h = dev.DCRemoval("complex_float64", 64, 2)
    x = rand_stream("complex_float64", 5000, 8)
    h.process(x)
    with pytest.raises(pcx._lib.PcxError):
        h.set_sizes(1 << 30, 1024)
    out = np.full_like(x, 5.0)
    with pytest.raises(pcx._lib.PcxError) as e:
        h.process(x, out=out)
    assert e.value.status == pcx._lib.ERR_STATE and np.all(out == 5.0)
    with pytest.raises(pcx._lib.PcxError):
        h.reset()
    h.set_sizes(64, 2)
    assert np.array_equal(h.process(x), dev.DCRemoval("complex_float64", 64, 2).process(x))


def test_block_keeps_its_sizes_when_the_device_cannot_hold_new_ones(dev):
    from pothoscomms_amd import blocks as B
    x = rand_stream("complex_float64", 3000, 12)
    blk = B.make("/comms/dc_removal", "complex_float64", module="filter")
    blk.call("setCascadeSize", 1024)
    with pytest.raises(Exception):
        blk.call("setAverageSize", 1 << 30)
    assert blk.call("getAverageSize") == 512 and blk.call("getCascadeSize") == 1024
    blk.activate()
    y, _, _, _, _ = blk.work(x, x.shape[0])
    assert np.array_equal(y, dev.DCRemoval("complex_float64", 512, 1024).process(x))


def test_process_checks_a_given_out(dev, pcx):
    h = dev.DCRemoval("int16", 8, 2)
    x = rand_stream("int16", 1000, 4)
    for bad in (np.zeros(999, np.int16), np.zeros(1000, np.int32), np.zeros(2000, np.int16)[::2]):
        with pytest.raises(pcx._lib.InvalidArgument):
            h.process(x, out=bad)


@pytest.mark.parametrize("dtype,C,D_fused", [("int64", 2, 1025), ("int8", 2, 1024), ("complex_int64", 1, 2049), ("float32", 4, 513),
                                             ("complex_float64", 2, 1025)])
def test_both_sides_of_the_fused_bound(dev, dtype, C, D_fused):
    """the halo C*(D-1) (C*D for int8) at 2048 runs fused, one sample more runs stage by stage.  A configuration takes one path by
    construction, so the two neighbours across the bound are each held to the fixture-verified restatement, over a stream cut in
    two calls (bit for bit for the integers)"""
    x = rand_stream(dtype, 70000, 9)
    for D in (D_fused, D_fused + 1):
        h = dev.DCRemoval(dtype, D, C)
        got = np.concatenate([h.process(x[:33333]), h.process(x[33333:])])
        assert_matches(got, x, dtype, D, C, "D=%d" % D)


def test_staged_path_across_chunks(dev):
    """int64 at a halo beyond the bound walks a call in chunks of 4 Mi samples: the carried accumulator crosses them"""
    n = (4 << 20) * 2 + 12345
    x = rand_stream("int64", n, 21)
    got = dev.DCRemoval("int64", 3000, 2).process(x)
    assert_matches(got, x, "int64", 3000, 2)
    y = rand_stream("complex_int16", (8 << 20) + 999, 22)
    got = dev.DCRemoval("complex_int16", 512, 2).process(y)
    assert_matches(got, y, "complex_int16", 512, 2)


@pytest.mark.parametrize("dtype", ["float32", "complex_float64"])
def test_nan_guard_bands_stay(dev, dtype):
    x = rand_stream(dtype, 50000, 2)
    G = 4096
    buf = np.full((x.shape[0] + 2 * G,) + x.shape[1:], np.nan, dtype=x.dtype)
    dev.DCRemoval(dtype, 512, 2).process(x, out=buf[G:G + x.shape[0]])
    assert np.all(np.isnan(buf[:G])) and np.all(np.isnan(buf[G + x.shape[0]:]))
    assert not np.any(np.isnan(buf[G:G + x.shape[0]]))


def _torch_of(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


@pytest.mark.parametrize("dtype", ["complex_float32", "complex_int16", "int8", "int32"])
def test_process_dev_on_a_torch_stream(dev, dtype):
    import torch
    x = rand_stream(dtype, 500000, 31)
    want = dev.DCRemoval(dtype, 300, 2).process(x)
    h = dev.DCRemoval(dtype, 300, 2)
    xd = _torch_of(x)
    yd = torch.empty_like(xd)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h.process_dev(xd[:200000], yd[:200000], 200000, stream=s)
        h.process_dev(xd[200000:], yd[200000:], 300000, stream=s)
    s.synchronize()
    assert np.array_equal(yd.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", ["complex_float32", "complex_int16"])
def test_graph_capture_replays(dev, dtype):
    import torch
    n = 1 << 18
    x = rand_stream(dtype, n, 41)
    ref = dev.DCRemoval(dtype)
    want = [ref.process(x) for _ in range(4)]
    h = dev.DCRemoval(dtype)
    xd = _torch_of(x)
    yd = torch.empty_like(xd)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        h.process_dev(xd, yd, n, stream=s)           # binds the stream, outside the capture
    s.synchronize()
    assert np.array_equal(yd.cpu().numpy(), want[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        h.process_dev(xd, yd, n, stream=s)
    for k in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(yd.cpu().numpy(), want[k]), k


def test_full_size_complex_float32_at_the_defaults(dev):
    """64 Mi samples through one call, checked in windows spread over the stream against the float64 restatement"""
    import torch
    n = 64 << 20
    D, C = 512, 2
    H = C * (D - 1)
    xd = torch.empty((n, 2), dtype=torch.float32, device="cuda:0")
    dev.fill_uniform_f32_dev(xd, seed=5)
    yd = torch.empty_like(xd)
    h = dev.DCRemoval("complex_float32")
    h.process_dev(xd, yd, n)
    torch.cuda.synchronize()
    for s in (0, 4095, 1 << 20, 33_333_333, n - 70000):
        lo = max(0, s - H)
        xs = xd[lo:s + 60000].cpu().numpy()
        want = M.restate(xs, "complex_float32", D, C)[s - lo:]
        got = yd[s:s + 60000].cpu().numpy()
        assert np.max(np.abs(got.astype(np.float64) - want)) <= 1e-6, s


@pytest.mark.parametrize("dtype", ["complex_float32", "complex_int16", "int64"])
def test_block_work_equals_the_handle(dev, dtype):
    from pothoscomms_amd import blocks as B
    x = rand_stream(dtype, 100000, 51)
    blk = B.make("/comms/dc_removal", dtype, module="filter")
    blk.call("setAverageSize", 200)
    blk.call("setCascadeSize", 3)
    blk.activate()
    outs, o = [], 0
    for s in (1, 199, 4099, 60000, 35701):
        y, consumed, produced, _, _ = blk.work(x[o:o + s], s)
        assert consumed == produced == s
        outs.append(y.copy())
        o += s
    want = dev.DCRemoval(dtype, 200, 3).process(x)
    assert np.array_equal(np.concatenate(outs), want)
    blk.call("setDevice", 0)               # a fresh handle on the named device: the carried state starts over
    y, _, _, _, _ = blk.work(x[:5000], 5000)
    assert np.array_equal(y, want[:5000])
