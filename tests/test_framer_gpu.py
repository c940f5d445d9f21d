"""GPU suite of /comms/preamble_framer and /comms/frame_insert: the framed stream of the C ABI, of the device-pointer call and of the
blocks against the model (tests/framer_model.py), and the loopback into the preamble correlator.  Every comparison is exact: on the
bytes of the output, so that the sign of a zero counts.  Every test runs under a time limit of its own: when it expires the process
ends there and nothing more is started on the device."""
import faulthandler
import os

import numpy as np
import pytest

import framer_model as M

pytestmark = pytest.mark.gpu

LIMIT_S = 300
CANARY = 0x5A
TYPES = ["uint8", "complex_float32", "complex_float64"]
ES = {"uint8": 1, "complex_float32": 8, "complex_float64": 16}
# (preamble, symbol width, header) per element type
SETUP = {"uint8": ([0, 1, 1, 1, 1, 0, 1], 1, False), "complex_float32": ([1, -1, 1j], 3, True), "complex_float64": ([1, 1, -1 + 0.5j], 2, True)}


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def shape(dev, dtype):
    tile = dev.Framer.geometry()[0] // ES[dtype]
    return tile, 3 * tile + 37


def stream(dtype, n, seed):
    rng = np.random.default_rng(seed)
    if dtype == "uint8":
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rng.standard_normal((n, 2)).astype(np.float32 if dtype == "complex_float32" else np.float64)


def make(dev, dtype, padding, setup=None):
    pre, width, header = setup or SETUP[dtype]
    f = dev.Framer(dtype, pre, width, header, header_id=0xA7, padding=padding)
    return f, M.Config(M.rows(f.preamble()[0]), width, header, 0xA7, padding)


def check(f, cfg, x, events, cap=None):
    """process() against both formulations of the model, with a canary behind the output length; returns the walk's result"""
    xr = M.rows(x)
    want, a = M.walk(xr, events, cfg, cap)
    want2, b = M.index_map(xr, events, cfg, cap)
    assert a.error is None and a[:6] == b[:6] and np.array_equal(want, want2)
    room = a.out_len + 64 if cap is None else cap + 64
    out = np.full((room,) + x.shape[1:], 0, x.dtype)
    out.view(np.uint8)[...] = CANARY
    r = f.process(x, events, out_cap=room - 64 if cap is not None else a.out_len, out=out)
    assert (r.consumed, r.out_len, r.cut, list(r.used)) == (a.consumed, a.out_len, a.cut, a.used), events[:8]
    assert [int(v) if u else 0 for v, u in zip(r.insert_at, a.used)] == a.insert_at and [int(v) if u else 0 for v, u in zip(r.shift, a.used)] == a.shift
    got = M.rows(out)
    bad = np.flatnonzero((got[:a.out_len] != want).any(axis=1))
    assert bad.size == 0, ("first wrong elements", bad[:8], got[bad[:2]], want[bad[:2]])
    assert np.all(got[a.out_len:] == CANARY), "the canary behind the output length"
    return a


@pytest.mark.parametrize("dtype", TYPES)
def test_no_labels_is_a_copy_and_an_empty_input_gives_nothing(dev, dtype):
    tile, n = shape(dev, dtype)
    f, cfg = make(dev, dtype, 5)
    x = stream(dtype, n, 1)
    assert check(f, cfg, x, []).out_len == n
    assert check(f, cfg, x, [(7, 1, "other", 0), (n - 1, 1, "other", 0)]).out_len == n
    assert check(f, cfg, x[:0], []).out_len == 0
    assert check(f, cfg, x[:0], [(0, 1, "start", 0)]).out_len == 0        # a label on an element that is not there
    assert check(f, cfg, x[:1], [(0, 1, "start", 0), (0, 1, "end", 0)]).consumed == 1
    f.close()


@pytest.mark.parametrize("dtype", TYPES)
def test_inserts_around_the_tile_seams_and_at_both_ends(dev, dtype):
    tile, n = shape(dev, dtype)
    f, cfg = make(dev, dtype, 13)
    x = stream(dtype, n, 2)
    for at in (0, tile - 1, tile, n - 1):
        check(f, cfg, x, [(at, 1, "start", 0x1234)])
        check(f, cfg, x, [(at, 1, "end", 0)])
        check(f, cfg, x, [(at, 1, "start", 77), (at, 1, "end", 0), (at, 1, "start", 78)])
    a = check(f, cfg, x, [(n - 9, 9, "end", 0)])                           # index + width == n: the padding ends the stream
    assert a.insert_at == [n] and a.out_len == n + 13
    check(f, cfg, x, [(n - 9, 1 << 40, "end", 0)])
    # all of it in one call, and an insert that begins exactly on a seam of the OUTPUT
    P = M.insert_len(cfg)
    check(f, cfg, x, [(0, 1, "start", 1), (tile - 1, 1, "end", 0), (tile, 1, "start", 2), (2 * tile - P - 13, 1, "start", 3), (n - 1, 1, "start", 4), (n - 1, 1, "end", 0)])
    f.close()


@pytest.mark.parametrize("plen", [1, 15, 16, 17, 33])
def test_byte_preambles_around_the_unit_size(dev, plen):
    tile, n = shape(dev, "uint8")
    pre = ((np.arange(plen) * 37 + 11) % 251 + 1).astype(np.uint8)
    f, cfg = make(dev, "uint8", 3, (pre, 1, False))
    x = stream("uint8", n, 3)
    # starts at every residue of 16, near a seam and far from one, some closer together than a unit
    at = [0, 1, 2, 19, 20, 50] + [tile - 40 + 7 * k for k in range(12)] + [2 * tile + 100 + 17 * k for k in range(16)] + [n - 2, n - 1]
    check(f, cfg, x, [(i, 1, "start", 0) for i in at] + [(n - 1, 1, "end", 0)])
    f.close()


@pytest.mark.parametrize("where", ["before_the_seam", "across_the_seam"])
def test_a_start_label_on_each_of_64_consecutive_bytes(dev, where):
    """preamble {9}: every output unit in the run is made of 16 segments"""
    tile, n = shape(dev, "uint8")
    f, cfg = make(dev, "uint8", 0, ([9], 1, False))
    x = stream("uint8", n, 4)
    # the run doubles in the output: 64 labels from i0 fill output [i0, i0 + 128)
    i0 = tile - 128 - 5 if where == "before_the_seam" else tile - 61
    a = check(f, cfg, x, [(i0 + k, 1, "start", 0) for k in range(64)])
    assert a.insert_at[0] == i0 and a.insert_at[-1] == i0 + 126 and (i0 + 128 < tile) == (where == "before_the_seam")
    # and more segments in a tile than a workgroup keeps on chip: the search in global memory
    lds = dev.Framer.geometry()[1]
    many = lds // 2 + 40
    a = check(f, cfg, x, [(tile + 3 * k, 1, "start", 0) for k in range(many)] + [(2 * tile + 5, 1, "start", 0)])
    assert a.out_len == n + many + 1
    f.close()


@pytest.mark.parametrize("dtype", TYPES)
def test_input_pointers_at_odd_byte_offsets(dev, dtype):
    import torch
    tile, n = shape(dev, dtype)
    es = ES[dtype]
    f, cfg = make(dev, dtype, 6)
    raw = np.random.default_rng(5).integers(0, 256, n * es + 64, dtype=np.uint8)
    rawd = torch.from_numpy(raw).cuda()
    assert rawd.data_ptr() % 16 == 0
    events = [(0, 1, "start", 5), (tile - 1, 2, "end", 0), (tile + 1, 1, "start", 6), (n - 1, 1, "start", 7)]
    for off in (1, 7, 15):
        xr = raw[off:off + n * es].reshape(n, es)
        want, a = M.walk(xr, events, cfg)
        outd = torch.full(((a.out_len + 8) * es,), CANARY, dtype=torch.uint8, device="cuda")
        r = f.process_dev(rawd[off:off + n * es], n, events, outd, a.out_len)
        torch.cuda.synchronize()
        got = outd.cpu().numpy().reshape(-1, es)
        assert (r.consumed, r.out_len) == (n, a.out_len) and np.array_equal(got[:a.out_len], want) and np.all(got[a.out_len:] == CANARY), off
        assert rawd.cpu().numpy().tobytes() == raw.tobytes()
    f.close()


@pytest.mark.parametrize("dtype", TYPES[1:])
def test_header_symbols_of_a_symbol_with_a_zero_component_keep_the_sign_of_zero(dev, dtype):
    tile, n = shape(dev, dtype)
    x = stream(dtype, 300, 6)
    ft = np.float32 if dtype == "complex_float32" else np.float64
    for last in ([1.0, 0.0], [0.0, -2.0], [-0.0, 3.0], [0.0, 0.0]):
        pre = np.array([[0.5, 0.5], last], ft)
        f = dev.Framer(dtype, pre, 2, True, header_id=0x55, padding=0)
        cfg = M.Config(M.rows(pre), 2, True, 0x55, 0)
        for length in (0, 0xFFF, 0xABCD):
            check(f, cfg, x, [(3, 1, "start", length), (200, 1, "start", length ^ 0x5A5)])
        r = f.process(x, [(0, 1, "start", 0xABCD)])
        hdr = r.out[4:4 + M.HEADER_BITS]
        bits = M.header_bits(0x55, 0xABCD)
        it = np.uint32 if ft == np.float32 else np.uint64
        plus, minus = pre[1].view(it), (-pre[1]).view(it)                  # unary minus: -0.0 for a zero component
        for k, bit in enumerate(bits):
            assert np.array_equal(hdr[k].view(it), plus if bit else minus), (last, k)
        assert not np.array_equal(plus, minus)                              # also for (0, 0): the two differ in their sign bits
        assert M.header_decode([int(np.array_equal(h.view(it), plus)) for h in hdr])[:2] == (0x55, 0xBCD)
        f.close()


def test_device_pointer_calls_back_to_back_on_one_stream(dev):
    import torch
    dtype = "complex_float32"
    tile, n = shape(dev, dtype)
    f, cfg = make(dev, dtype, 4)
    x = stream(dtype, n, 7)
    xd = torch.from_numpy(x).cuda()
    P = M.insert_len(cfg)
    calls = [[(k * 97, 1, "start", k) for k in range(1, 20)], [], [(5, 1, "start", 1), (tile, 3, "end", 0)], [(n - 1, 1, "end", 0)], [(0, 1, "start", 9)]]
    outs = [torch.full((n + 20 * (P + 4) + 16, 2), float("nan"), dtype=torch.float32, device="cuda") for _ in calls]
    st = torch.cuda.Stream()
    results = []
    with torch.cuda.stream(st):
        for events, o in zip(calls, outs):                                 # five calls, no host synchronisation between them: the table slots rotate
            results.append(f.process_dev(xd, n, events, o, o.shape[0] - 16, stream=st))
    st.synchronize()
    for events, o, r in zip(calls, outs, results):
        want, a = M.walk(M.rows(x), events, cfg)
        got = M.rows(o.cpu().numpy())
        assert (r.consumed, r.out_len) == (n, a.out_len) and np.array_equal(got[:a.out_len], want), events[:3]
        assert np.all(np.isnan(o.cpu().numpy()[a.out_len:]))
    # a call whose output would overlap its input is refused
    with pytest.raises(ValueError, match="overlaps"):
        f.process_dev(xd, n, [], xd[8:], n - 8)
    f.close()


def post(B, labels):
    return [B.Label(i, index, data, width) for i, index, width, data in labels]


@pytest.mark.parametrize("dtype", TYPES)
def test_blocks_cut_by_a_small_output_buffer_equal_the_uncut_model(dev, dtype):
    from pothoscomms_amd import blocks as B
    tile, n = shape(dev, dtype)
    n = tile + 37
    x = stream(dtype, n, 8)
    header = dtype != "uint8"
    b = B.make("/comms/preamble_framer", module="framer") if not header else B.make("/comms/frame_insert", dtype, module="framer")
    pre = [0, 1, 1, 1, 1, 0] if not header else [1, 1, -1]
    b.call("setPreamble", pre)
    if header:
        b.call("setSymbolWidth", 4)
        b.call("setHeaderId", 0xA7)
    b.call("setFrameEndId", "frameEnd")
    b.call("setPaddingSize", 13)
    width = 4 if header else 1
    pre_rows = M.rows(np.asarray(pre, np.uint8) if not header else np.asarray(pre).astype(np.complex64 if dtype == "complex_float32" else np.complex128))
    cfg = M.Config(pre_rows, width, header, 0xA7, 13)
    # (id, index, width, data): data * width is the header's length; a string does not convert and gives 0
    labels = [("frameStart", 0, 1, 300), ("note", 0, 1, "hello"), ("frameEnd", 500, 1, None), ("frameStart", 501, 2, 1000), ("tick", 700, 1, 2.5),
              ("frameEnd", tile - 2, 4, None), ("frameStart", tile + 1, 1, "text"), ("frameEnd", n - 1, 1, None)]
    events = [(i, w, "start" if name == "frameStart" else "end" if name == "frameEnd" else "other",
               (d * w if isinstance(d, int) else 0) & 0xFFFF) for name, i, w, d in labels]
    want, a = M.walk(M.rows(x), events, cfg)
    want_labels = [(labels[k][0], at, labels[k][2], labels[k][3]) for k, at in M.expected_labels(events, a)]
    for cap in (a.out_len + 5, 4096 // ES[dtype] + 203):
        pos, outs, got_labels, produced, calls = 0, [], [], 0, 0
        left = list(labels)
        while pos < n:
            out, consumed, made, _, posted = b.work(x[pos:], cap, labels=post(B, left), label_cap=32)
            assert consumed > 0 and made <= cap
            outs.append(M.rows(out).copy())
            got_labels += [(l.id, produced + l.index, l.width, l.data) for l in posted]
            pos, produced, calls = pos + consumed, produced + made, calls + 1
            left = [(i, at - consumed, w, d) for i, at, w, d in left if at >= consumed]
        assert np.array_equal(np.concatenate(outs), want) and got_labels == want_labels, cap
        assert (calls == 1) == (cap >= a.out_len)
    # setDevice creates the handle again and keeps the settings
    b.call("setDevice", 0)
    out, consumed, made, _, posted = b.work(x, a.out_len, labels=post(B, labels), label_cap=32)
    assert (consumed, made) == (n, a.out_len) and np.array_equal(M.rows(out), want)
    assert [(l.id, l.index, l.width, l.data) for l in posted] == want_labels
    b.close()


def test_block_ids_the_start_id_is_tested_first_and_an_empty_end_id_matches_an_empty_label(dev):
    from pothoscomms_amd import blocks as B
    x = stream("uint8", 100, 9)
    b = B.make("/comms/preamble_framer", module="framer")
    b.call("setPreamble", [7, 8])
    b.call("setPaddingSize", 3)
    cfg = M.Config(M.rows(np.array([7, 8], np.uint8)), 1, False, 0x55, 3)
    # the default end id is empty: the label without an id is an end label, the one named frameEnd is not
    labels = [("frameStart", 10, 1, None), ("", 20, 1, None), ("frameEnd", 30, 1, None)]
    out, consumed, made, _, posted = b.work(x, 200, labels=post(B, labels))
    want, a = M.walk(M.rows(x), [(10, 1, "start", 0), (20, 1, "end", 0), (30, 1, "other", 0)], cfg)
    assert np.array_equal(M.rows(out), want) and [(l.id, l.index) for l in posted] == [("frameStart", 10), ("", 25), ("frameEnd", 35)]
    # equal ids: both labels are start labels
    b.call("setFrameStartId", "x")
    b.call("setFrameEndId", "x")
    out, consumed, made, _, posted = b.work(x, 200, labels=post(B, [("x", 10, 1, None), ("x", 50, 1, None)]))
    want, a = M.walk(M.rows(x), [(10, 1, "start", 0), (50, 1, "start", 0)], cfg)
    assert np.array_equal(M.rows(out), want) and made == 104 and [(l.id, l.index) for l in posted] == [("x", 10), ("x", 52)]
    # an insert that no output buffer of this size can take is an error, not a stall
    with pytest.raises(ValueError, match=r"need 3 output elements, the output buffer holds 2"):
        b.work(x, 2, labels=post(B, [("x", 0, 1, None)]))
    b.close()


def test_loopback_the_correlator_finds_every_frame_the_framer_made(dev):
    """payload symbols 2 and 3 only, a preamble of zeros and ones: no window of the payload, and no window that straddles a frame start,
    is the preamble, so with threshold 0 the labels fall exactly at each frame start plus the preamble length"""
    tile, n = shape(dev, "uint8")
    pre = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1], np.uint8)
    payload = np.random.default_rng(10).integers(2, 4, n, dtype=np.uint8)
    starts = [0, 5, 999, tile - 11, tile, 2 * tile + 3, n - 1]
    f = dev.Framer("uint8", pre)
    r = f.process(payload, [(s, 1, "start", 0) for s in starts])
    assert r.out_len == n + len(starts) * pre.size
    idx, positions, matches = dev.PreambleCorrelator(pre, threshold=0).process(r.out)
    assert matches == len(starts) and positions == r.out_len - pre.size
    assert list(idx) == [int(at) + pre.size for at in r.insert_at] == [s + (k + 1) * pre.size for k, s in enumerate(starts)]
    f.close()


# ---- the recorded reference: tests/golden/framer.npz, what the reference's own work() posted (tests/golden/make_framer_golden.py).
# Every recorded case outside DESIGN.md 18's "a head never runs backwards" (the fixture's `backward` flag; tests/test_framer_cpu.py holds
# the list of their names and that model and reference differ there and nowhere else)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "framer.npz")


@pytest.fixture(scope="module")
def golden():
    return M.golden_cases(GOLDEN)


def typed(rows, dtype):
    return M.unrows(rows, None) if dtype == "uint8" else np.ascontiguousarray(rows).view(np.float32 if dtype == "complex_float32" else np.float64).reshape(-1, 2)


def recorded_labels(c):
    """what the reference posted, as the blocks' labels: (id, index, width, data)"""
    assert all(c["labels"][k][2] == w and M.DATA_KINDS.index(None if c["labels"][k][3] is None else "integer" if isinstance(c["labels"][k][3], int) else "string") == kind
               for k, _, w, kind in c["posted"])
    return [(c["labels"][k][0], at, w, c["labels"][k][3]) for k, at, w, _ in c["posted"]]


@pytest.mark.parametrize("dtype", TYPES)
def test_process_process_dev_and_the_blocks_equal_every_recorded_case_of_the_reference(dev, golden, dtype):
    import torch
    from pothoscomms_amd import blocks as B
    tile_bytes, cases, _ = golden
    assert dev.Framer.geometry()[0] == tile_bytes, "the kernel's output tile changed: record tests/golden/framer.npz again for the new tile"
    mine = [c for c in cases if c["dtype"] == dtype]
    assert mine and any(c["backward"] for c in mine)
    header = dtype != "uint8"
    blk = B.make("/comms/frame_insert", dtype, module="framer") if header else B.make("/comms/preamble_framer", module="framer")
    es, ran = ES[dtype], 0
    for c in mine:
        if c["backward"]:
            continue
        cfg, ev, n, want = c["cfg"], c["events"], c["n"], c["out"]
        x = typed(c["x"], dtype)
        f = dev.Framer(dtype, c["preamble"], cfg.width, cfg.header, header_id=cfg.header_id, padding=cfg.padding)
        # the host-pointer call
        r = f.process(x, ev, out_cap=want.shape[0])
        assert (r.consumed, r.out_len, r.cut) == (c["consumed"], want.shape[0], False), c["name"]
        assert np.array_equal(M.rows(r.out), want), (c["name"], np.flatnonzero((M.rows(r.out) != want).any(axis=1))[:8])
        posted = [(k, ev[k][0] + int(r.shift[k])) for k in range(len(ev)) if r.used[k]]
        assert posted == [p[:2] for p in c["posted"]], c["name"]
        # the device-pointer call, a canary behind the output
        xd = torch.from_numpy(x).cuda()
        outd = torch.full(((want.shape[0] + 8) * es,), CANARY, dtype=torch.uint8, device="cuda")
        r = f.process_dev(xd, n, ev, outd, want.shape[0])
        torch.cuda.synchronize()
        got = outd.cpu().numpy().reshape(-1, es)
        assert (r.consumed, r.out_len) == (c["consumed"], want.shape[0]) and np.array_equal(got[:want.shape[0]], want) and np.all(got[want.shape[0]:] == CANARY), c["name"]
        assert [(k, ev[k][0] + int(r.shift[k])) for k in range(len(ev)) if r.used[k]] == posted, c["name"]
        f.close()
        # the block: its own classification of the ids and its own length field from the labels' data
        pre = c["preamble"]
        blk.call("setPreamble", np.ascontiguousarray(pre.astype(np.float64)).view(np.complex128).reshape(-1) if header else pre)
        if header:
            blk.call("setSymbolWidth", cfg.width)
            blk.call("setHeaderId", cfg.header_id)
        blk.call("setFrameStartId", c["start_id"])
        blk.call("setFrameEndId", c["end_id"])
        blk.call("setPaddingSize", cfg.padding)
        out, consumed, made, _, labels = blk.work(x, want.shape[0], labels=post(B, c["labels"]), label_cap=max(64, len(ev)))
        assert (consumed, made) == (c["consumed"], want.shape[0]) and np.array_equal(M.rows(out), want), c["name"]
        assert [(l.id, l.index, l.width, l.data) for l in labels] == recorded_labels(c), c["name"]
        ran += 1
    blk.close()
    assert ran == sum(not c["backward"] for c in mine)
