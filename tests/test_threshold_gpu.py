"""GPU suite of /comms/threshold: transition indices, counts, entry states and per-element states of the C ABI, the device-pointer
calls and the block against the model (tests/threshold_model.py).  Every comparison is exact.  Every test runs under a time limit of
its own: when it expires the process ends there and nothing more is started on the device."""
import faulthandler

import numpy as np
import pytest

import threshold_model as M

pytestmark = pytest.mark.gpu

LIMIT_S = 420
# (activation, deactivation): above, equal to (the default) and below the deactivation level -- the last makes the toggle band
PAIRS = {"above": (40, -25), "equal": (0, 0), "below": (-25, 40)}
CANARY = 0x5A


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def shape(dev):
    tile = dev.Threshold.geometry()[0]
    return tile, 3 * tile + 37


def cast(x, dtype):
    return (x if "float" in dtype else np.rint(x)).astype(dtype)


def noise(rng, dtype, pair, n):
    return cast(rng.uniform(min(pair) - 60, max(pair) + 60, n), dtype)


def dense(dtype, pair, n):
    """every element is a transition: inside the toggle band where there is one, else far above and far below the levels in turn"""
    act, deact = pair
    lo, hi = (act + 1, deact - 1) if act < deact else (-100, 100)
    x = np.where(np.arange(n) % 2 == 0, hi, lo)
    return x.astype(dtype)


def sparse(dtype, pair, n, tile):
    """crossings on the last element of a tile, the first of the next, and the stream's first and last elements.  Between them the
    value keeps either state where the levels leave such a value (activation >= deactivation) and clears it where they do not."""
    act, deact = pair
    x = np.full(n, 0 if act >= deact else -100, dtype=np.float64)
    at = [0, tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1]
    x[at] = [100, -100, 100, -100, 100, -100] if act >= deact else 100
    return x.astype(dtype), at


def still(dtype, pair, n):
    """nothing changes an ACTIVE state: a keep where the levels leave one, else a value at or above the deactivation level"""
    act, deact = pair
    return np.full(n, 0 if act >= deact else 100).astype(dtype)


def check(t, x, pair, entry):
    """states() and process() of handle t, entered in `entry`, against the model; returns the model's result"""
    idx, n, e, final, s = M.run(x, pair[0], pair[1], entry)
    t.set_state(entry)
    got = t.states(x)
    assert got.dtype == np.uint8 and np.array_equal(got, s), ("states", np.nonzero(got != s)[0][:8])
    assert t.state() == entry                      # states() leaves the carried state alone
    out = np.full(x.size, CANARY, x.dtype)
    gi, gn, ge = t.process(x, out=out)
    assert (gn, ge) == (n, e) and gi.dtype == np.uint64 and np.array_equal(gi, idx), ("process", gn, n, ge, e)
    assert out.tobytes() == x.tobytes() and t.state() == final
    return idx, n, final


@pytest.mark.parametrize("dtype", M.TYPES)
def test_grid_of_level_pairs_and_inputs(dev, dtype):
    tile, n = shape(dev)
    rng = np.random.default_rng(400 + M.TYPES.index(dtype))
    for name, pair in PAIRS.items():
        t = dev.Threshold(dtype, *pair)
        assert tuple(int(v) for v in t.levels()) == pair and t.state() == 0
        for entry in (0, 1):
            _, cnt, _ = check(t, noise(rng, dtype, pair, n), pair, entry)
            assert cnt > n // 8, (name, cnt)
        xs, at = sparse(dtype, pair, n, tile)
        idx, cnt, _ = check(t, xs, pair, 0)
        assert set(at) <= set(int(i) for i in idx) or pair[0] < pair[1]
        assert {0, tile - 1 if pair[0] >= pair[1] else tile, n - 1} & set(int(i) for i in idx)
        check(t, xs, pair, 1)
        idx, cnt, _ = check(t, dense(dtype, pair, n), pair, 0)
        assert cnt == n and np.array_equal(idx, np.arange(n, dtype=np.uint64))
        # the state set by set_state crosses three tiles that do not change it
        idx, cnt, final = check(t, still(dtype, pair, n), pair, 1)
        assert (cnt, final) == (0, 1)
        t.close()


@pytest.mark.parametrize("dtype", M.TYPES)
def test_a_stream_cut_into_calls_equals_the_single_call(dev, dtype):
    tile, n = shape(dev)
    rng = np.random.default_rng(500 + M.TYPES.index(dtype))
    for name, pair in PAIRS.items():
        x = noise(rng, dtype, pair, n)
        want, cnt, _, final, _ = M.run(x, pair[0], pair[1], 0)
        t = dev.Threshold(dtype, *pair)
        one = t.process(x)
        assert np.array_equal(one[0], want) and one[1:] == (cnt, 0) and t.state() == final
        t.reset()
        assert t.state() == 0
        entries = []

        def work(buf):
            before = t.state()
            idx, k, e = t.process(buf)
            assert e == before and k == idx.size
            entries.append(e)
            return idx
        got = M.run_cuts(work, x, [1, 0, 37, tile - 1, 2, tile + 1, None])
        assert np.array_equal(got, want) and t.state() == final, name
        assert entries[1] == entries[2]                 # the empty call left the state alone
        t.reset()
        again = t.process(x)
        assert np.array_equal(again[0], one[0]) and again[1:] == one[1:]
        t.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_special_float_values_and_nan_levels(dev, dtype):
    tile, n = shape(dev)
    rng = np.random.default_rng(600)
    x = rng.uniform(-1, 1, n).astype(dtype)
    x[rng.integers(0, n, n // 4)] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dtype), n // 4)
    x[[0, tile - 1, tile, n - 1]] = [np.nan, np.inf, -np.inf, -0.0]
    for pair in ((0.0, 0.0), (-0.0, 0.0), (0.5, -0.5), (-0.5, 0.5), (np.inf, -np.inf), (-np.inf, np.inf)):
        t = dev.Threshold(dtype, *pair)
        for entry in (0, 1):
            check(t, x, pair, entry)
        t.close()
    # zeros of either sign against levels of either sign: nothing is above or below
    z = np.where(rng.integers(0, 2, n) == 0, 0.0, -0.0).astype(dtype)
    t = dev.Threshold(dtype, -0.0, 0.0)
    for entry in (0, 1):
        assert check(t, z, (-0.0, 0.0), entry)[1] == 0
    t.close()
    # a NaN level compares false with everything: that kind of transition never happens
    for pair, entry, most in (((np.nan, 0.0), 0, 0), ((np.nan, np.nan), 1, 0), ((np.nan, np.nan), 0, 0), ((0.0, np.nan), 0, 1), ((np.nan, 0.0), 1, 1)):
        t = dev.Threshold(dtype, *pair)
        assert np.isnan(t.levels()[0]) or np.isnan(t.levels()[1])
        _, cnt, _ = check(t, x, pair, entry)
        assert cnt <= most and (cnt == most or most == 0), (pair, entry, cnt)
        t.close()


@pytest.mark.parametrize("dtype", ["int64", "int32", "int16", "int8"])
def test_integer_extremes(dev, dtype):
    tile, n = shape(dev)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(700)
    x = rng.choice(np.array([info.min, info.max, info.min + 1, info.max - 1, 0, -1], dtype), n)
    x[[0, tile - 1, tile, n - 1]] = [info.max, info.min, info.max, info.min]
    # x > MAX and x < MIN never hold
    t = dev.Threshold(dtype, info.max, info.min)
    assert tuple(int(v) for v in t.levels()) == (info.max, info.min)
    for entry in (0, 1):
        assert check(t, x, (info.max, info.min), entry)[1] == 0
    t.close()
    for pair in ((info.min, info.max), (info.max - 1, info.min + 1), (info.min, info.min), (info.max, info.max)):
        t = dev.Threshold(dtype, *pair)
        for entry in (0, 1):
            check(t, x, pair, entry)
        t.close()


def test_int64_levels_beyond_the_doubles(dev):
    tile, n = shape(dev)
    lv = 2**62 + 1
    x = np.resize(np.array([2**62, 2**62 + 1, 2**62 + 2], np.int64), n)
    assert np.unique(x.astype(np.float64)).size == 1          # in double the three values and the level are one number
    t = dev.Threshold("int64", lv, lv)
    assert tuple(int(v) for v in t.levels()) == (lv, lv)
    idx, cnt, _ = check(t, x, (lv, lv), 0)
    assert n % 3 == 1 and cnt == 2 * (n // 3) and int(idx[0]) == 2 and int(idx[1]) == 3
    t.set_levels(-lv, -lv)
    check(t, -x, (-lv, -lv), 1)
    t.close()


@pytest.mark.parametrize("dtype", ["int8", "float32", "float64"])
def test_more_transitions_than_the_index_buffer_holds(dev, dtype):
    import torch
    tile, n = shape(dev)
    pair = PAIRS["below"]
    x = dense(dtype, pair, n)
    xd = torch.from_numpy(x).cuda()
    t = dev.Threshold(dtype, *pair)
    for cap in (0, 1, tile, n - 1):
        # host pointers: the first cap indices, the full count, the state advances (n is odd: the dense stream leaves it toggled)
        t.reset()
        idx, cnt, entry = t.process(x, cap=cap)
        assert (cnt, entry, t.state()) == (n, 0, n % 2) and np.array_equal(idx, np.arange(cap, dtype=np.uint64))
        # device pointers: nothing is written behind cap
        t.reset()
        idxd = torch.full((n + 16,), -1, dtype=torch.int64, device="cuda")
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        t.process_dev(xd, n, idxd, cap, counts)
        torch.cuda.synchronize()
        got = idxd.cpu().numpy()
        assert counts.cpu().tolist() == [n, n, 0] and t.state() == n % 2
        assert np.array_equal(got[:cap], np.arange(cap)) and np.all(got[cap:] == -1), cap
    t.close()


@pytest.mark.parametrize("dtype", M.TYPES)
def test_device_pointers_at_any_alignment(dev, dtype):
    import torch
    tile, n = shape(dev)
    pair = PAIRS["below"]
    rng = np.random.default_rng(800 + M.TYPES.index(dtype))
    pad = 64
    x = noise(rng, dtype, pair, n + pad)
    es = x.dtype.itemsize
    xd0 = torch.from_numpy(x).cuda()
    assert xd0.data_ptr() % 16 == 0
    t = dev.Threshold(dtype, *pair)
    for off in (0, 1, 3, 17):
        assert off == 0 or (off * es) % 16 != 0
        xs = x[off:off + n]
        want, cnt, _, final, s = M.run(xs, pair[0], pair[1], 0)
        canary = np.frombuffer(bytes([CANARY]) * es, x.dtype)[0]
        for mode in ("separate", "in place", "none"):
            xd = xd0.clone()
            outd = torch.from_numpy(np.full(n + 2 * pad, canary, x.dtype)).cuda()
            idxd = torch.full((n + 16,), -1, dtype=torch.int64, device="cuda")
            counts = torch.full((5,), -1, dtype=torch.int64, device="cuda")
            xin = xd[off:off + n]
            out = {"separate": outd[pad + off:pad + off + n], "in place": xin, "none": None}[mode]
            t.reset()
            t.process_dev(xin, n, idxd, n, counts[1:4], out=out)
            torch.cuda.synchronize()
            assert counts.cpu().tolist() == [-1, n, cnt, 0, -1] and t.state() == final, (off, mode)
            got = idxd.cpu().numpy()
            assert np.array_equal(got[:cnt].astype(np.uint64), want) and np.all(got[cnt:] == -1), (off, mode)
            assert xd.cpu().numpy().tobytes() == x.tobytes(), (off, mode)                 # the input, and what lies around it
            o = outd.cpu().numpy()
            if mode == "separate":
                assert o[pad + off:pad + off + n].tobytes() == xs.tobytes()
                o[pad + off:pad + off + n] = canary
            assert np.all(o == canary) or np.all(o.view(np.uint8) == CANARY), (off, mode)
        # the states, canaried on both sides; the carried state stays
        t.set_state(1)
        sd = torch.full((n + 2 * pad,), CANARY, dtype=torch.uint8, device="cuda")
        t.states_dev(xd0[off:off + n], n, sd[pad + off:pad + off + n])
        torch.cuda.synchronize()
        got = sd.cpu().numpy()
        assert np.array_equal(got[pad + off:pad + off + n], M.states_scan(xs, pair[0], pair[1], 1)) and t.state() == 1
        assert np.all(got[:pad + off] == CANARY) and np.all(got[pad + off + n:] == CANARY)
    # two calls back to back on one stream, no host synchronisation between them: the second starts in the state the first left
    half = tile + 11
    xs = x[:n]
    want = M.run(xs, pair[0], pair[1], 0)
    first = M.run(xs[:half], pair[0], pair[1], 0)
    second = M.run(xs[half:], pair[0], pair[1], first[3])
    t.reset()
    ia, ib = (torch.full((n,), -1, dtype=torch.int64, device="cuda") for _ in range(2))
    ca, cb = (torch.zeros(3, dtype=torch.int64, device="cuda") for _ in range(2))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t.process_dev(xd0[:half], half, ia, n, ca, stream=stream)
        t.process_dev(xd0[half:n], n - half, ib, n, cb, stream=stream)
    stream.synchronize()
    assert ca.cpu().tolist() == [half, first[1], 0] and cb.cpu().tolist() == [n - half, second[1], first[3]]
    joined = np.concatenate([ia.cpu().numpy()[:first[1]], ib.cpu().numpy()[:second[1]] + half]).astype(np.uint64)
    assert np.array_equal(joined, want[0]) and t.state() == want[3]
    t.close()


def labels_of(idx, entry, act_id, deact_id):
    ids = [act_id if k else deact_id for k in M.kinds(idx.size, entry)]
    return [(i, int(at)) for i, at in zip(ids, idx) if i]


@pytest.mark.parametrize("dtype", M.TYPES)
def test_block_posts_the_models_labels(dev, dtype):
    from pothoscomms_amd import blocks as B
    tile, n = shape(dev)
    pair = PAIRS["below"]
    rng = np.random.default_rng(900 + M.TYPES.index(dtype))
    x = noise(rng, dtype, pair, n)
    want = M.run(x, pair[0], pair[1], 0)
    b = B.make("/comms/threshold", dtype, module="utility")
    b.call("setActivationLevel", pair[0])
    b.call("setDeactivationLevel", pair[1])
    b.call("setActivationId", "rise")
    b.call("setDeactivationId", "fall")
    b.activate()

    def work(buf, entry):
        out, consumed, produced, _, labels = b.work(buf, buf.size, label_cap=buf.size + 8)
        assert (consumed, produced) == (buf.size, buf.size) and out.tobytes() == buf.tobytes()
        assert all(l.width == 1 and l.data is None for l in labels)
        return [(l.id, l.index) for l in labels]
    got = work(x, 0)
    assert got == labels_of(want[0], 0, "rise", "fall") and [i for _, i in got] == sorted(i for _, i in got) and len(got) == want[1]
    # the next call continues from the state the first left; activate() starts over
    x2 = noise(rng, dtype, pair, tile + 5)
    assert work(x2, want[3]) == labels_of(M.run(x2, pair[0], pair[1], want[3])[0], want[3], "rise", "fall")
    b.activate()
    assert work(x, 0) == got
    # an empty activation ID drops that kind and nothing else: the state changes all the same
    b.call("setActivationId", "")
    b.activate()
    assert work(x, 0) == labels_of(want[0], 0, "", "fall") == [p for p in got if p[0] == "fall"]
    b.call("setActivationId", "rise")
    b.call("setDeactivationId", "")
    b.activate()
    assert work(x, 0) == [p for p in got if p[0] == "rise"]
    # fewer output elements than input elements: k = min(in, out)
    b.call("setDeactivationId", "fall")
    b.activate()
    out, consumed, produced, _, labels = b.work(x, tile + 1, label_cap=n)
    assert (consumed, produced) == (tile + 1, tile + 1) and [(l.id, l.index) for l in labels] == [p for p in got if p[1] <= tile]
    b.close()


@pytest.mark.parametrize("dtype", ["int8", "float64"])
def test_block_grows_its_index_buffer_and_restores_the_state(dev, dtype):
    from pothoscomms_amd import blocks as B
    tile, n = shape(dev)
    pair = PAIRS["below"]
    x = dense(dtype, pair, n)
    assert n > 4096 and n % 2 == 1
    b = B.make("/comms/threshold", dtype, module="utility")
    b.call("setActivationLevel", pair[0])
    b.call("setDeactivationLevel", pair[1])
    b.call("setActivationId", "rise")
    b.call("setDeactivationId", "fall")
    b.activate()
    out, consumed, produced, _, labels = b.work(x, n, label_cap=n + 8)
    assert (consumed, produced) == (n, n) and out.tobytes() == x.tobytes()
    # every label exactly once: a call repeated from the wrong state would start with "fall"
    assert [(l.id, l.index) for l in labels] == [("rise" if i % 2 == 0 else "fall", i) for i in range(n)]
    # n is odd: the block is active now, and the next work() starts with a deactivation
    out, consumed, produced, _, labels = b.work(x[:101], 101, label_cap=256)
    assert [(l.id, l.index) for l in labels] == [("fall" if i % 2 == 0 else "rise", i) for i in range(101)]
    b.activate()
    out, consumed, produced, _, labels = b.work(x[:101], 101, label_cap=256)
    assert [(l.id, l.index) for l in labels] == [("rise" if i % 2 == 0 else "fall", i) for i in range(101)]
    b.close()


def test_slice_seam_int8(dev):
    """The suite's one long test: a call of slice + tile + 5 elements (64 Mi and a little) takes a second slice."""
    tile, slc = dev.Threshold.geometry()
    n = slc + tile + 5
    pair = PAIRS["below"]                               # activation -25, deactivation 40
    rng = np.random.default_rng(1000)
    x = np.full(n, 100, np.int8)                        # at or above both levels: sets
    x[:tile] = noise(rng, "int8", pair, tile)
    x[-(tile + 5):] = noise(rng, "int8", pair, tile + 5)
    x[slc - 40] = -100                                  # a deactivation in front of the seam ...
    x[slc - 30] = 100
    x[slc - 7:slc + 9] = 0                              # ... a run inside the toggle band across it ...
    x[slc + 20] = -100                                  # ... and transitions behind it
    want, cnt, _, final, s = M.run(x, pair[0], pair[1], 0)
    assert set(range(slc - 7, slc + 9)) <= set(int(i) for i in want) and cnt < 3 * tile
    t = dev.Threshold("int8", *pair)
    got = t.states(x)
    assert np.array_equal(got, s), np.nonzero(got != s)[0][:8]
    idx, k, entry = t.process(x, cap=4 * tile)
    assert (k, entry) == (cnt, 0) and np.array_equal(idx, want) and t.state() == final
    t.close()
