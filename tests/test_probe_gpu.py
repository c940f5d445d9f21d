"""GPU suite of /comms/signal_probe: every type and mode against the exact truth within the derived bounds (tests/probe_model.py), the
batch against single calls, byte addresses and positions in a batch, special values, the block through the runner, and the stream
argument.  "The same" means the same 64 bits of both doubles throughout.  Every test runs under a time limit of its own: when it
expires the process ends there and nothing more is started on the device."""
import faulthandler

import numpy as np
import pytest

import probe_model as M

pytestmark = pytest.mark.gpu

LIMIT_S = 300
CANARY = -7.25
FLOAT_TYPES = ["float64", "float32", "complex_float64", "complex_float32"]
OFFSETS = (0, 1, 4, 15, 17)


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    t.cuda.set_device(0)
    return t


def pair(v):
    return (v.real, v.imag) if isinstance(v, complex) else (float(v), 0.0)


def bits(v):
    """the 64 bits of each double of a value, a pair or an array of pairs"""
    if isinstance(v, (float, complex)):
        v = pair(v)
    return np.ascontiguousarray(np.asarray(v, np.float64)).view(np.uint64).copy()


def paths(p):
    """a window for each way through the kernels: a wave alone (up to 64 units, and beyond them as the four waves of the tree), a
    workgroup alone, several slices"""
    tile, slc, switch = p.geometry()
    return (3, 257, tile - 3, switch + 5)


def to_device(torch, x, offset=0, tail=0):
    """the bytes of x at byte `offset` of a fresh device buffer (`tail` spare bytes behind): (tensor, device address of the bytes)"""
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    buf = torch.zeros(offset + raw.size + tail + 16, dtype=torch.uint8, device="cuda")
    buf[offset:offset + raw.size].copy_(torch.from_numpy(raw.copy()))
    return buf, buf.data_ptr() + offset


def batch_dev(torch, p, x, offset=0, guard=3):
    """windows_dev over x placed at a byte offset: (pairs, the guard pairs behind them)"""
    n = x.shape[0]
    nw = -(-n // p.window)
    buf, addr = to_device(torch, x, offset)
    values = torch.full((nw + guard, 2), CANARY, dtype=torch.float64, device="cuda")
    p.windows_dev(addr, n, values)
    torch.cuda.synchronize()
    out = values.cpu().numpy()
    del buf
    return out[:nw], out[nw:]


# ---- every type, mode and length against the truth
@pytest.mark.parametrize("dtype", M.TYPES)
def test_every_mode_against_the_truth_within_the_bounds(dev, dtype):
    p = dev.SignalProbe(dtype)
    ns = M.lengths(p.geometry()) + ([M.BIG] if dtype in M.BIG_TYPES else [])
    worst = {"RMS": 0.0, "MEAN": 0.0}
    for n in ns:
        x = M.make_input(dtype, n)
        for window in ((n, n + 5) if n < 300 else (n,)):          # a window longer than the call reduces what there is (SignalProbe.cpp:127)
            p.set_window(window)
            for mode in M.MODES:
                p.set_mode(mode)
                got, consumed = p.process(x)
                assert consumed == n and type(got) is (complex if M.is_complex(dtype) else float)
                got = pair(got)
                true, lim = M.case(dtype, n, mode)
                for k in (0, 1):
                    err = abs(got[k] - true[k])
                    if lim[k] > 0:
                        worst[mode] = max(worst[mode], err / lim[k])
                    assert err <= lim[k], (dtype, n, mode, k, got[k], true[k], err, lim[k])
                if mode == "VALUE":
                    assert np.array_equal(bits(got), bits(true)), (dtype, n)
                if M.sum_is_exact(dtype, mode):
                    # every term and every partial sum is an integer below 2^53: the order of the additions cannot matter
                    assert np.array_equal(bits(got), bits(M.model(x, mode))), (dtype, n, mode, got)
                    if mode == "MEAN":
                        assert np.array_equal(bits(got), bits(true)), (dtype, n, got, true)
    print("%s: worst error / bound: RMS %.3f, MEAN %.3f over %d lengths" % (dtype, worst["RMS"], worst["MEAN"], len(ns)))
    p.close()


# ---- the batch
@pytest.mark.parametrize("dtype", M.TYPES)
def test_the_batch_equals_single_calls(dev, torch, dtype):
    p = dev.SignalProbe(dtype)
    for W in paths(p):
        p.set_window(W)
        for r in (0, 1, W - 1):
            n = 7 * W + r
            x = M.make_input(dtype, n, 1)
            nw = -(-n // W)
            assert nw == (7 if r == 0 else 8)
            for mode in M.MODES:
                p.set_mode(mode)
                singles = []
                at = 0
                while at < n:
                    v, consumed = p.process(x[at:])
                    assert consumed == min(W, n - at)
                    singles.append(pair(v))
                    at += consumed
                assert len(singles) == nw
                got, guard = batch_dev(torch, p, x)
                assert got.shape == (nw, 2) and np.array_equal(bits(got), bits(singles)), (dtype, W, r, mode)
                assert np.all(guard == CANARY), (dtype, W, r, mode, guard)
                host = p.windows(x)
                assert host.shape == (nw,) and np.array_equal(bits(np.array([pair(v.item()) for v in host])), bits(singles))
    p.close()


# ---- byte addresses and positions
@pytest.mark.parametrize("dtype", M.TYPES)
def test_any_byte_address_and_any_position_give_the_same_bits(dev, torch, dtype):
    p = dev.SignalProbe(dtype)
    for W in paths(p):
        p.set_window(W)
        window = M.make_input(dtype, W, 2)
        filler = M.make_input(dtype, 7 * W, 3)
        for mode in M.MODES:
            p.set_mode(mode)
            want = bits(p.process(window)[0])
            seen = []
            for pos in (0, 5):
                x = filler.copy()
                x[pos * W:(pos + 1) * W] = window
                for off in OFFSETS:
                    got, guard = batch_dev(torch, p, x, off)
                    assert np.all(guard == CANARY)
                    seen.append(bits(got[pos]))
                    # ... and the windows around it are the filler's, wherever they lie
                    if pos == 5 and off == OFFSETS[-1]:
                        base, _ = batch_dev(torch, p, filler)
                        assert np.array_equal(bits(np.delete(got, pos, 0)), bits(np.delete(base, pos, 0)))
            assert all(np.array_equal(s, want) for s in seen), (dtype, W, mode, want, seen)
    p.close()


@pytest.mark.parametrize("dtype", M.TYPES)
def test_the_two_paths_give_the_same_bits(dev, torch, dtype):
    """the remainder window of a batch of long windows runs through the large-window path's slices and join; alone, the same elements
    take the small-window path (a wave, or a workgroup): the tree is the same, so are the bits"""
    p = dev.SignalProbe(dtype)
    tile, slc, switch = p.geometry()
    W = switch + 5
    units = 16 // (M.scalar_of(dtype).itemsize * (2 if M.is_complex(dtype) else 1))
    for r in (1, 3, 64 * units, 64 * units + 1, 257 * units, tile - 1, tile):
        x = M.make_input(dtype, W + r, 9)
        for mode in M.MODES:
            p.set_mode(mode)
            p.set_window(W)
            got, _ = batch_dev(torch, p, x)
            assert got.shape == (2, 2)
            alone, consumed = p.process(x[W:])              # r elements: a window of the small-window path
            assert consumed == r and np.array_equal(bits(got[1]), bits(alone)), (dtype, r, mode, got[1], alone)
            p.set_window(r)
            again, _ = batch_dev(torch, p, np.concatenate([x[W:], x[W:]]))
            assert np.array_equal(bits(again[0]), bits(alone)) and np.array_equal(bits(again[1]), bits(alone)), (dtype, r, mode)
    p.close()


def test_one_window_alone_and_among_many_windows_in_a_launch(dev, torch):
    """the number of windows in the launch leaves a window's bits alone: 1, 2, 5 and 4099 windows (more than one launch group of the
    large-window path would need gigabytes: the wave-owned path stands for many)"""
    for dtype, W in (("complex_float32", 1024), ("int16", 5), ("float64", 8)):
        p = dev.SignalProbe(dtype, "RMS", W)
        x = M.make_input(dtype, 4099 * W, 4)
        for mode in ("RMS", "MEAN"):
            p.set_mode(mode)
            full, _ = batch_dev(torch, p, x)
            for count in (1, 2, 5):
                part, _ = batch_dev(torch, p, x[:count * W])
                assert np.array_equal(bits(part), bits(full[:count])), (dtype, mode, count)
            again, _ = batch_dev(torch, p, x)
            assert np.array_equal(bits(again), bits(full))                     # and from run to run
        p.close()


# ---- special values
@pytest.mark.parametrize("dtype", FLOAT_TYPES)
def test_special_values_on_the_float_types(dev, dtype):
    p = dev.SignalProbe(dtype)
    sc = M.scalar_of(dtype)
    cplx = M.is_complex(dtype)

    def run(x, mode):
        p.set_mode(mode)
        v, consumed = p.process(x)
        assert consumed == x.shape[0]
        return pair(v)

    for W in paths(p):
        p.set_window(W)
        base = np.array(M.make_input(dtype, W, 5))
        base = np.where(np.abs(base) > 1e6, sc.type(1.5), base).astype(sc)       # (moderate values around the planted ones)
        for at in sorted({0, W // 2, W - 1}):
            x = base.copy()
            x.reshape(-1)[at * (2 if cplx else 1)] = np.nan
            assert np.isnan(run(x, "RMS")[0]) and np.isnan(run(x, "MEAN")[0]), (dtype, W, at)
            x.reshape(-1)[at * (2 if cplx else 1)] = np.inf
            assert run(x, "RMS") == (np.inf, 0.0) and run(x, "MEAN")[0] == np.inf, (dtype, W, at)
            if W > 1:
                x.reshape(-1)[((at + 1) % W) * (2 if cplx else 1)] = -np.inf
                assert run(x, "RMS") == (np.inf, 0.0) and np.isnan(run(x, "MEAN")[0]), (dtype, W, at)
        if sc == np.float64:
            x = np.full(base.shape, 1e200, sc)
            assert run(x, "RMS") == (np.inf, 0.0) == M.model(x, "RMS")           # the squares overflow, as the reference's do
            assert abs(run(x, "MEAN")[0] - 1e200) <= 1e186                        # (the sum itself stays finite)
        zeros = np.zeros(base.shape, sc)
        for mode in M.MODES:
            assert np.array_equal(bits(run(zeros, mode)), bits((0.0, 0.0))), (dtype, W, mode)
        minus = np.full(base.shape, -0.0, sc)
        for mode in M.MODES:
            assert np.array_equal(bits(run(minus, mode)), bits(M.model(minus, mode))), (dtype, W, mode, run(minus, mode))
        assert np.array_equal(bits(run(minus, "VALUE")[0:1]), bits(-0.0)[0:1]) and np.array_equal(bits(run(minus, "MEAN")), bits((0.0, 0.0)))
    p.close()


# ---- the block
def make(dtype):
    from pothoscomms_amd import blocks as B
    return B.make("/comms/signal_probe", dtype, module="probe")


def feed(b, x):
    """one work() on a host port buffer of the block's own manager; returns what it consumed"""
    arr, _ = b.port_buffer(0, x.shape, x.dtype)
    arr[...] = x
    outs, consumed, produced = b.work_ports([arr], [])
    assert outs == [] and produced == []
    return consumed[0]


@pytest.mark.parametrize("dtype", ["float32", "complex_float32", "complex_int16", "int8", "complex_float64", "int64"])
def test_the_block_consumes_a_window_and_holds_its_value(dev, dtype):
    b = make(dtype)
    p = dev.SignalProbe(dtype)
    x = M.make_input(dtype, 700, 6)
    b.activate()
    for mode in M.MODES:
        for window in (1, 100, 700, 5000):
            b.call("setMode", mode)
            b.call("setWindow", window)
            p.set_mode(mode)
            p.set_window(window)
            assert feed(b, x) == min(window, 700)
            want, consumed = p.process(x)
            assert consumed == min(window, 700)
            got = b.call("value")
            assert type(got) is type(want) and np.array_equal(bits(got), bits(want)), (dtype, mode, window, got, want)
    # rate 0.0: three calls, three values
    b.call("setMode", "MEAN")
    b.call("setWindow", 200)
    p.set_mode("MEAN")
    p.set_window(200)
    values = []
    for k in range(3):
        assert feed(b, x[200 * k:]) == 200
        values.append(b.call("value"))
        assert np.array_equal(bits(values[-1]), bits(p.process(x[200 * k:])[0]))
    assert len({bits(v).tobytes() for v in values}) == 3
    # a mode that names no calculation: the elements are consumed, the value stays
    b.call("setMode", "PEAK")
    assert feed(b, x) == 200 and np.array_equal(bits(b.call("value")), bits(values[-1]))
    # the device applied again: the handle is a new one, mode and window are the old ones
    b.call("setMode", "RMS")
    b.call("setWindow", 333)
    b.call("setDevice", 0)
    assert (b.call("getMode"), b.call("getWindow"), b.call("getDevice"), b.reserve()) == ("RMS", 333, 0, 333)
    p.set_mode("RMS")
    p.set_window(333)
    assert feed(b, x) == 333 and np.array_equal(bits(b.call("value")), bits(p.process(x)[0]))
    b.close()
    p.close()


def test_the_rate_holds_calculations_back_and_the_signals_carry_the_value(dev):
    a, b = make("float32"), make("float64")
    a.connect_signal("valueChanged", b, "setRate")
    x = M.make_input("float32", 300, 7)
    p = dev.SignalProbe("float32", "RMS", 100)
    want = [p.process(x[100 * k:])[0] for k in range(3)]
    a.call("setMode", "RMS")
    a.call("setWindow", 100)
    # rate 0.0: every call calculates and signals
    a.activate()
    for k in range(3):
        b.call("setRate", -1.0)
        assert feed(a, x[100 * k:]) == 100
        assert a.call("value") == want[k] and b.call("getRate") == want[k]
    # one calculation in a thousand seconds: the first call after activate() calculates, the next two only consume
    a.call("setRate", 1e-3)
    a.activate()
    b.call("setRate", -1.0)
    assert feed(a, x) == 100 and a.call("value") == want[0] and b.call("getRate") == want[0]
    b.call("setRate", -1.0)
    for k in (1, 2):
        assert feed(a, x[100 * k:]) == 100
        assert a.call("value") == want[0] and b.call("getRate") == -1.0        # no calculation, no signal
    # an unknown mode still signals, with the value as it was
    a.call("setRate", 0.0)
    a.call("setMode", "PEAK")
    assert feed(a, x[100:]) == 100 and a.call("value") == want[0] and b.call("getRate") == want[0]
    # probeValue -> valueTriggered
    c = make("float64")
    a.connect_signal("valueTriggered", c, "setRate")
    assert c.call("getRate") == 0.0
    a.call("probeValue")
    assert c.call("getRate") == want[0]
    for blk in (a, b, c):
        blk.close()
    p.close()


# ---- the stream argument
@pytest.mark.parametrize("dtype", ["complex_float32", "int8", "float64"])
def test_a_stream_of_the_callers_gives_the_same_bits(dev, torch, dtype):
    p = dev.SignalProbe(dtype)
    side = torch.cuda.Stream()
    for W in paths(p):
        p.set_window(W)
        n = 3 * W + 2
        x = M.make_input(dtype, n, 8)
        buf, addr = to_device(torch, x)
        torch.cuda.synchronize()
        for mode in M.MODES:
            p.set_mode(mode)
            out = []
            for stream in (0, side):
                values = torch.full((4 + 2, 2), CANARY, dtype=torch.float64, device="cuda")
                one = torch.full((2, 2), CANARY, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                p.windows_dev(addr, n, values, stream=stream)
                assert p.process_dev(addr, n, one, stream=stream) == W
                torch.cuda.synchronize()
                v, o = values.cpu().numpy(), one.cpu().numpy()
                assert np.all(v[4:] == CANARY) and np.all(o[1] == CANARY)
                assert np.array_equal(bits(o[0]), bits(v[0]))
                out.append(bits(v[:4]))
            assert np.array_equal(out[0], out[1]), (dtype, W, mode)
            assert np.array_equal(out[0][0], bits(p.process(x)[0]))
        del buf
    p.close()
