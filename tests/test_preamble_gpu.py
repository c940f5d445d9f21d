"""GPU suite of /comms/preamble_correlator: indices, counts and distances of the C ABI, the block and the device-pointer calls
against the model (tests/preamble_model.py).  Every comparison is exact.  Every test runs under a time limit of its own: when it
expires the process ends there and nothing more is started on the device."""
import faulthandler
import os

import numpy as np
import pytest

import preamble_model as M

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 6, 31, 32, 33, 64, 65, 255, 1024]
LIMIT_S = 420


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def thresholds(P):
    return sorted({0, 1, P, 8 * P - 1, 8 * P})


def seam_stream(rng, pre, tile, width=8):
    """random symbols over three tiles and a part of a fourth, the preamble planted at the first and the last position, across both
    tile seams, right in front of a seam and right behind one (where they do not overlap)"""
    P = pre.size
    n = 3 * tile + P + 37 + P
    x = rng.integers(0, 1 << width, n, dtype=np.uint8)
    at = [0, tile - P // 2 - 1, 2 * tile - 1, n - P - 1]
    if P < tile // 4:
        at += [tile + 1 + P, 2 * tile - P - 1 - P, 3 * tile]
    return M.plant(x, pre, at), at


def check_call(c, pre, x, thr_list):
    d = M.distances_plain(pre, x)
    got = c.distances(x)
    assert got.dtype == np.uint32 and np.array_equal(got, d), ("distances", pre.size, np.nonzero(got != d)[0][:8] if got.size == d.size else got.size)
    for thr in thr_list:
        c.set_threshold(thr)
        want = M.matches_of(d, thr, pre.size)
        idx, npos, nm = c.process(x)
        assert (npos, nm) == (d.size, want.size), (pre.size, thr)
        assert idx.dtype == np.uint64 and np.array_equal(idx, want), (pre.size, thr)
    return d


@pytest.mark.parametrize("P", LENGTHS)
def test_grid_of_lengths_and_thresholds_across_the_tile_seams(dev, P):
    tile, _, longest = dev.PreambleCorrelator.geometry()
    assert P <= longest
    rng = np.random.default_rng(200 + P)
    for width in (1, 8):
        pre = rng.integers(0, 1 << width, P, dtype=np.uint8)
        pre[0] |= 1
        x, at = seam_stream(rng, pre, tile, 8)
        c = dev.PreambleCorrelator(pre)
        assert c.plan() == dev._lib.PRE_PLANES and c.threshold() == 1
        d = check_call(c, pre, x, thresholds(P))
        assert all(d[a] == 0 for a in at) and d.size - 1 in at and 0 in at
        c.close()


@pytest.mark.parametrize("P", [1, 33, 64, 1024])
def test_device_pointers_at_every_byte_alignment(dev, P):
    import torch
    tile = dev.PreambleCorrelator.geometry()[0]
    rng = np.random.default_rng(300 + P)
    pre = rng.integers(0, 4, P, dtype=np.uint8)
    x, _ = seam_stream(rng, pre, tile, 2)
    c = dev.PreambleCorrelator(pre, threshold=P // 2)
    xd = torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), x])).cuda()
    for shift in (0, 1, 5, 8, 15):
        xs = x[shift:]
        d = M.distances_plain(pre, xs)
        want = M.matches_of(d, P // 2, P)
        view = xd[16 + shift:]
        idx = torch.zeros(max(1, d.size), dtype=torch.int64, device="cuda")
        counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((d.size + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        dist = torch.zeros(d.size, dtype=torch.int32, device="cuda")
        c.process_dev(view, xs.size, idx, d.size, counts, out=out[shift:])
        c.distances_dev(view, xs.size, dist)
        torch.cuda.synchronize()
        assert counts.tolist() == [d.size, want.size], (P, shift)
        assert np.array_equal(idx[:want.size].cpu().numpy().astype(np.uint64), want), (P, shift)
        assert np.array_equal(dist.cpu().numpy().astype(np.uint32), d), (P, shift)
        o = out.cpu().numpy()
        assert np.array_equal(o[shift:shift + d.size], xs[:d.size]) and np.all(o[:shift] == 0xEE) and np.all(o[shift + d.size:] == 0xEE), (P, shift)
    c.close()


def test_all_ones_and_all_zero_input(dev):
    tile = dev.PreambleCorrelator.geometry()[0]
    rng = np.random.default_rng(5)
    for P in (6, 64, 257):
        for pre in (rng.integers(0, 256, P, dtype=np.uint8), np.zeros(P, np.uint8), np.full(P, 0xFF, np.uint8)):
            c = dev.PreambleCorrelator(pre)
            for fill in (0x00, 0xFF):
                x = np.full(2 * tile + P + 3, fill, np.uint8)
                d = check_call(c, pre, x, [0, int(M.distances_plain(pre, x[:P + 1])[0]), 8 * P])
                assert np.all(d == d[0])
            c.close()


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_one_to_eight_active_planes(dev, width):
    tile = dev.PreambleCorrelator.geometry()[0]
    rng = np.random.default_rng(40 + width)
    for P in (16, 100):
        for shift in (0, 8 - width):                      # the planes at the bottom and at the top of the byte
            pre = (rng.integers(0, 1 << width, P, dtype=np.uint8) << shift).astype(np.uint8)
            pre[:width] |= ((1 << np.arange(width)) << shift).astype(np.uint8)           # every one of the planes is active
            active = int(np.bitwise_or.reduce(pre))
            assert bin(active).count("1") == width
            x = M.plant(rng.integers(0, 256, 2 * tile + 500, dtype=np.uint8), pre, [7, tile - 5, 2 * tile + 499 - P])
            noisy = x.copy()
            noisy[tile - 5 + 3] ^= 0x81                                    # one bit at each end of the byte
            c = dev.PreambleCorrelator(pre)
            check_call(c, pre, x, [0, 1, 2, 3 * P])
            check_call(c, pre, noisy, [0, 1, 2])
            c.close()


def test_dirty_upper_bits_never_match_a_bit_preamble_at_threshold_0(dev):
    rng = np.random.default_rng(3)
    pre = rng.integers(0, 2, 24, dtype=np.uint8)
    pre[0] = 1
    bits = M.plant(rng.integers(0, 2, 9000, dtype=np.uint8), pre, [100, 4090, 8000])
    c = dev.PreambleCorrelator(pre, threshold=0)
    clean = c.process(bits)[0]
    assert np.array_equal(clean, M.matches_plain(pre, 0, bits)[0]) and {124, 4114, 8024} <= set(int(i) for i in clean)
    dirty = bits | 0x80
    assert c.process(dirty)[2] == 0
    c.set_threshold(23)
    assert c.process(dirty)[2] == 0
    c.set_threshold(24)
    assert np.array_equal(c.process(dirty)[0], clean)
    c.close()


def test_index_capacity_smaller_than_the_match_count(dev):
    tile = dev.PreambleCorrelator.geometry()[0]
    rng = np.random.default_rng(6)
    pre = rng.integers(0, 2, 10, dtype=np.uint8)
    x = rng.integers(0, 2, 3 * tile + 77, dtype=np.uint8)
    want, N, nm = M.matches_plain(pre, 3, x)
    assert nm > tile // 4                                  # matches in every tile, more than most of the capacities below
    c = dev.PreambleCorrelator(pre, threshold=3)
    for cap in (0, 1, 63, tile // 8 + 1, nm - 1, nm, nm + 5):
        idx, npos, got = c.process(x, cap=cap)
        assert (npos, got) == (N, nm) and np.array_equal(idx, want[:cap]), cap
    c.close()


def test_preamble_longer_than_the_tiles_halo_takes_the_byte_plan(dev):
    tile, _, longest = dev.PreambleCorrelator.geometry()
    rng = np.random.default_rng(8)
    P = longest + 3
    pre = rng.integers(0, 256, P, dtype=np.uint8)
    x = M.plant(rng.integers(0, 256, 2 * tile + 100 + P, dtype=np.uint8), pre, [0, tile - 2, 2 * tile + 99])
    c = dev.PreambleCorrelator(pre)
    assert c.plan() == dev._lib.PRE_BYTES
    check_call(c, pre, x, [0, 3 * P, 4 * P, 8 * P])
    c.set_preamble(pre[:longest])
    assert c.plan() == dev._lib.PRE_PLANES
    check_call(c, pre[:longest], x, [0, 4 * longest])
    c.close()


# ---- the block
def block_labels(blk, buf, pid):
    out, consumed, produced, reserve, labels = blk.work(buf, buf.size, label_cap=max(64, buf.size))
    assert consumed == produced == out.size and np.array_equal(out, buf[:consumed])           # the output bytes are the input
    assert all(l.id == pid and l.data is None and l.width == 1 for l in labels)
    return consumed, reserve, [l.index for l in labels]


@pytest.mark.parametrize("P", [6, 64, 200])
def test_stream_cut_into_work_calls_equals_the_one_shot_result(dev, P):
    from pothoscomms_amd import blocks as B
    rng = np.random.default_rng(60 + P)
    pre = rng.integers(0, 2, P, dtype=np.uint8)
    pre[0] = pre[-1] = 1
    n = 30000
    x = M.plant(rng.integers(0, 2, n, dtype=np.uint8), pre, [0, 4096 - P // 2, 9000, 9000 + P, 20000 - 1, n - P - 1])
    want, N, nm = M.matches_plain(pre, 1, x)
    assert nm >= 6
    for path in ("/comms/preamble_correlator", "/blocks/preamble_correlator"):
        blk = B.make(path, module="correlator")
        blk.call("setPreamble", pre)
        blk.call("setThreshold", 1)
        blk.call("setFrameStartId", "sof")
        # cuts shorter than, equal to and longer than the preamble
        cuts = [1, P - 1, P, P, P + 1, 1, 2 * P, 5000, 3, 8192, P]
        cuts.append(n - sum(cuts))
        assert cuts[-1] > 0

        def work(buf):
            consumed, reserve, idx = block_labels(blk, buf, "sof")
            assert reserve == P + 1                        # asked for on every call, also when nothing could be done
            return consumed, idx
        labels, done = M.run_cuts(work, x, cuts, P)
        assert done == N and np.array_equal(labels, want)
        blk.close()


def test_block_posts_every_label_when_they_outnumber_its_index_buffer(dev):
    from pothoscomms_amd import blocks as B
    blk = B.make("/comms/preamble_correlator", module="correlator")
    blk.call("setThreshold", 8)                            # preamble {1}: every position matches
    x = np.random.default_rng(9).integers(0, 256, 20001, dtype=np.uint8)
    consumed, reserve, idx = block_labels(blk, x, "frameStart")
    assert (consumed, reserve) == (20000, 2)
    want = M.matches_plain([1], 8, x)[0]
    assert np.array_equal(np.array(idx, np.uint64), want) and want.size > 4096
    blk.close()


def test_block_refuses_a_device_that_does_not_exist(dev):
    import torch
    from pothoscomms_amd import _lib, blocks as B
    blk = B.make("/comms/preamble_correlator", module="correlator")
    blk.call("setPreamble", [1, 0, 1])
    with pytest.raises(_lib.InvalidArgument, match="device"):
        blk.call("setDevice", torch.cuda.device_count())
    blk.call("setDevice", 0)
    assert blk.call("getDevice") == 0 and blk.call("getPreamble") == [1, 0, 1] and blk.call("getThreshold") == 1
    consumed, reserve, idx = block_labels(blk, np.array([1, 0, 1, 0, 0, 1, 1, 1, 1], np.uint8), "frameStart")
    assert (consumed, reserve, idx) == (6, 4, [int(i) for i in M.matches_plain([1, 0, 1], 1, [1, 0, 1, 0, 0, 1, 1, 1, 1])[0]])
    with pytest.raises(_lib.InvalidArgument):
        blk.call("setPortSlabBytes", 1)
    blk.close()


# ---- large calls on the device
@pytest.mark.parametrize("width", [1, 8])
def test_64mi_symbols_against_the_torch_model_on_the_device(dev, width):
    import torch
    tile, slc, _ = dev.PreambleCorrelator.geometry()
    P = 64
    rng = np.random.default_rng(70 + width)
    pre = rng.integers(0, 1 << width, P, dtype=np.uint8)
    pre[0] |= 1
    n = (64 << 20) + tile + P + 5                          # the slice seam lies inside
    assert n - P > slc
    g = torch.Generator(device="cuda").manual_seed(71)
    x = torch.randint(0, 1 << width, (n,), dtype=torch.uint8, device="cuda", generator=g)
    pt = torch.from_numpy(pre).cuda()
    at = [0, 12345, slc - P // 2, slc + 2 * P, n - P - 1]
    for a in at:
        x[a:a + P] = pt
    thr = 20 if width == 1 else 220                      # about one random position in 10^3 matches
    c = dev.PreambleCorrelator(pre, threshold=thr)
    N = n - P
    dist = torch.zeros(N, dtype=torch.int32, device="cuda")
    cap = 1 << 22
    idx = torch.zeros(cap, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    c.distances_dev(x, n, dist)
    c.process_dev(x, n, idx, cap, counts)
    torch.cuda.synchronize()
    npos, nm = counts.tolist()
    assert npos == N and len(at) <= nm <= cap
    assert all(int(dist[a]) == 0 for a in at)
    got = M.torch_check(pre, thr, x, dist=dist, idx=idx[:nm])
    assert got == (N, nm, 0, 0), got
    c.close()


def test_one_call_beyond_2_32_positions(dev):
    import torch
    tile, slc, _ = dev.PreambleCorrelator.geometry()
    P = 48
    pre = np.random.default_rng(11).integers(0, 2, P, dtype=np.uint8)
    pre[0] = pre[-1] = 1                                   # no shifted window over a zero background can match
    edge = 1 << 32
    n = edge + 3 * tile + P + 11
    at = [0, 77, slc - 5, edge - 3 * P, edge - P // 2, edge + P, edge + 1000, n - P - 1]
    x = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pt = torch.from_numpy(pre).cuda()
    for a in at:
        x[a:a + P] = pt
    c = dev.PreambleCorrelator(pre, threshold=0)
    idx = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    c.process_dev(x, n, idx, 64, counts)
    torch.cuda.synchronize()
    assert counts.tolist() == [n - P, len(at)]
    assert idx[:len(at)].tolist() == [a + P for a in at] and int(idx[len(at)]) == -1
    c.close()


def test_graph_capture_replays_equal_to_the_eager_result(dev):
    import torch
    tile = dev.PreambleCorrelator.geometry()[0]
    rng = np.random.default_rng(12)
    P, n, cap = 32, 5 * tile + 100, 4096
    pre = rng.integers(0, 2, P, dtype=np.uint8)
    streams = [M.plant(rng.integers(0, 2, n, dtype=np.uint8), pre, list(rng.integers(0, n - P, 9))) for _ in range(3)]
    c = dev.PreambleCorrelator(pre, threshold=2)
    xd = torch.from_numpy(streams[0]).cuda()
    idx = torch.zeros(cap, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c.process_dev(xd, n, idx, cap, counts, out=out, stream=s)          # the first call, outside the graph: the stream is bound
    s.synchronize()
    eager = (counts.tolist(), idx.cpu().numpy().copy())
    want0 = M.matches_plain(pre, 2, streams[0])
    assert eager[0] == [want0[1], want0[2]] and np.array_equal(eager[1][:want0[2]].astype(np.uint64), want0[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        c.process_dev(xd, n, idx, cap, counts, out=out, stream=s)
    for x in streams[1:]:                                  # two replays, each on fresh input
        xd.copy_(torch.from_numpy(x).cuda())
        idx.zero_()
        counts.zero_()
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, N, nm = M.matches_plain(pre, 2, x)
        assert counts.tolist() == [N, nm] and np.array_equal(idx[:nm].cpu().numpy().astype(np.uint64), want)
        assert np.array_equal(out[:N].cpu().numpy(), x[:N])
        e_idx, e_n, e_nm = c.process(x)                    # the eager call on the same input
        assert (e_n, e_nm) == (N, nm) and np.array_equal(e_idx, want)
    c.close()


# ---- the recorded reference: tests/golden/preamble.npz, what the reference's own work() posted (tests/golden/make_preamble_golden.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preamble.npz")
FAMILIES = ["grid", "fill", "planes", "dirty", "cuts"]


@pytest.fixture(scope="module")
def golden():
    return M.golden_cases(GOLDEN)


def test_recorded_cases_are_sorted_into_families_and_the_tile_is_the_recorded_one(dev, golden):
    tile, halo, cases = golden
    got_tile, _, longest = dev.PreambleCorrelator.geometry()
    assert (got_tile, longest) == (tile, halo), "the kernel's tile or halo changed: record tests/golden/preamble.npz again for the new shapes"
    assert {c["name"].split("/")[0] for c in cases} == set(FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_process_distances_and_the_block_equal_every_recorded_call_of_the_reference(dev, golden, family):
    from pothoscomms_amd import blocks as B
    tile, halo, cases = golden
    assert dev.PreambleCorrelator.geometry()[0] == tile, "record tests/golden/preamble.npz again for the new tile"
    blk = B.make("/comms/preamble_correlator", module="correlator")
    blk.call("setFrameStartId", "sof")
    ran = 0
    for case in cases:
        if case["name"].split("/")[0] != family:
            continue
        pre, x, P = case["preamble"], case["x"], case["preamble"].size
        c = dev.PreambleCorrelator(pre)
        assert c.plan() == (dev._lib.PRE_BYTES if P > halo else dev._lib.PRE_PLANES)
        blk.call("setPreamble", pre)

        def check(buf, call, dist):
            thr, handed, consumed, reserve, forwarded, want = call
            assert handed == buf.size
            # the distances decide the labels: positions at or under the threshold are the recorded ones, no other
            assert dist.size == consumed and np.array_equal(np.flatnonzero(dist <= thr).astype(np.uint64) + np.uint64(P), want), (case["name"], thr)
            c.set_threshold(thr)
            idx, npos, nm = c.process(buf)
            assert (npos, nm) == (consumed, want.size) and idx.dtype == np.uint64 and np.array_equal(idx, want), (case["name"], thr)
            blk.call("setThreshold", thr)
            got = block_labels(blk, buf, "sof")
            assert got[:2] == (consumed, reserve) and consumed == forwarded, (case["name"], thr)
            assert np.array_equal(np.array(got[2], np.uint64), want), (case["name"], thr)

        if case["cuts"] is None:
            dist = c.distances(x)
            for call in case["calls"]:
                check(x, call, dist)
        else:
            calls = iter(case["calls"])

            def work(buf):
                call = next(calls)
                check(buf, call, c.distances(buf))
                return call[2], call[5]
            M.run_cuts(work, x, case["cuts"], P)
            assert next(calls, None) is None
        c.close()
        ran += 1
    blk.close()
    assert ran == sum(c["name"].split("/")[0] == family for c in cases) > 0
