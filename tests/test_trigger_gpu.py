"""GPU suite of /comms/wave_trigger: the search against the model (tests/trigger_model.py) at the seams of its tiles, for every type and
at odd byte addresses; the capture byte for byte; and the block through the runner on buffers in device memory against the calls
recorded from the reference (tests/golden/trigger.npz).  "Equal" means the same bits throughout.  Every test runs under a time limit
of its own: when it expires the process ends there and nothing more is started on the device."""
import faulthandler

import numpy as np
import pytest

import trigger_model as M

pytestmark = pytest.mark.gpu

LIMIT_S = 120
CANARY = 0xA5
ALL_TYPES = ["float64", "float32", "int64", "int32", "int16", "int8", "complex_float64", "complex_float32", "complex_int64", "complex_int32", "complex_int16",
             "complex_int8", "uint64", "uint32", "uint16", "uint8"]


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


@pytest.fixture(scope="module")
def golden():
    return M.load_golden()


@pytest.fixture(scope="module")
def blocks(pcx):
    from pothoscomms_amd import blocks as b
    b.load("trigger")
    return b


def to_device(torch, x, offset=0, tail=0):
    """the bytes of x at byte `offset` of a fresh device buffer, CANARY around them: (tensor, device address of the bytes)"""
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    buf = torch.full((offset + raw.size + tail + 16,), CANARY, dtype=torch.uint8, device="cuda")
    buf[offset:offset + raw.size].copy_(torch.from_numpy(raw.copy()))
    return buf, buf.data_ptr() + offset


def f32bits(v):
    return int(np.float32(v).view(np.uint32))


def f64bits(v):
    return int(np.float64(v).view(np.uint64))


def expected(x, dtype, level, slope, start):
    hit = M.search(M.search_floats(x, dtype), level, slope, start)
    if hit is None:
        return None
    i, y0, y1 = hit
    return i, f32bits(y0), f32bits(y1), f64bits(M.position_of(i, y0, y1, level))


def as_bits(hit):
    return None if hit is None else (hit[0], f32bits(hit[1]), f32bits(hit[2]), f64bits(hit[3]))


def check(torch, dev, x, dtype, level, slope, start, offset=0, want="model"):
    """the host-pointer call on device memory (searched where it lies) and the device call: both equal the model"""
    t = dev.Trigger(dtype, level, slope)
    buf, addr = to_device(torch, x, offset)
    exp = expected(x, dtype, level, slope, start)
    if want != "model":
        assert (exp[0] if exp else None) == want
    assert as_bits(t.search(addr, start, len(x))) == exp
    hit = torch.full((24 + 8,), CANARY, dtype=torch.uint8, device="cuda")
    t.search_dev(addr, len(x), start, hit)
    torch.cuda.synchronize()
    raw = hit.cpu().numpy()
    assert (raw[24:] == CANARY).all()
    i, found = int(raw[0:8].view(np.uint64)[0]), int(raw[16:24].view(np.uint64)[0])
    y0, y1 = raw[8:12].view(np.float32)[0], raw[12:16].view(np.float32)[0]
    if exp is None:
        assert (found, i, f32bits(y0), f32bits(y1)) == (0, 0, 0, 0)
    else:
        assert (found, i, f32bits(y0), f32bits(y1)) == (1,) + exp[:3]
    t.close()
    del buf
    return exp


def sizes(dev):
    T = dev.Trigger("float32").geometry()
    return T, (3 * T + 5, 64 * T)


# ---- the search at the seams
@pytest.mark.parametrize("which", [0, 1])
def test_search_seams(torch, dev, which):
    T, ns = sizes(dev)
    n = ns[which]
    x = np.zeros(n, np.float32)
    check(torch, dev, x, "float32", 0.5, "POS", 0, want=None)                          # no crossing
    x[T], x[T + 1] = 1.0, 1.0
    check(torch, dev, x, "float32", 0.5, "POS", 0, want=T - 1)                         # the pair that straddles the first tile's end
    check(torch, dev, x, "float32", 0.5, "POS", 7, want=T - 1)
    check(torch, dev, x, "float32", 0.5, "POS", T - 1, want=T - 1)                     # the first pair at `from`
    check(torch, dev, x, "float32", 0.5, "POS", T, want=None)                          # `from` behind the only crossing
    check(torch, dev, x, "float32", 0.5, "NEG", 0, want=T + 1)
    check(torch, dev, x, "float32", 0.5, "LEVEL", T, want=T + 1)
    y = np.zeros(n, np.float32)
    y[n - 1] = 2.0
    check(torch, dev, y, "float32", 0.5, "POS", 0, want=n - 2)                         # the last pair
    check(torch, dev, y, "float32", 0.5, "POS", n - 2, want=n - 2)
    check(torch, dev, y, "float32", 0.5, "POS", n - 1, want=None)                      # no pair in the range
    y[5], y[6] = 0.25, 0.75
    check(torch, dev, y, "float32", 0.5, "POS", 5, want=5)                             # the first pair at `from`, a fraction
    check(torch, dev, y, "float32", 0.5, "POS", 6, want=n - 2)


def test_search_the_lower_of_two_wins(torch, dev):
    T, (_, n) = sizes(dev)
    x = np.zeros(n, np.float32)
    x[40 * T + 17], x[3 * T + 900] = 1.0, 1.0
    check(torch, dev, x, "float32", 0.5, "POS", 0, want=3 * T + 899)
    check(torch, dev, x, "float32", 0.5, "POS", 3 * T + 900, want=40 * T + 16)
    x[:] = 1.0
    x[1::2] = 0.0
    for start in (0, 1, 63, 64, T - 1, T, 5 * T + 3):                                  # every pair a crossing: the least one, from run to run
        for _ in range(3):
            check(torch, dev, x, "float32", 0.5, "POS", start, want=start + (1 - start % 2))


def test_search_nan_and_second_equals_level(torch, dev):
    T, (n, _) = sizes(dev)
    x = np.zeros(n, np.float32)
    x[T - 2:T + 3] = [0.0, np.nan, 1.0, np.nan, 0.0]
    check(torch, dev, x, "float32", 0.5, "LEVEL", 0, want=None)
    x[2 * T + 9:2 * T + 12] = [0.25, 0.5, 0.5]
    exp = check(torch, dev, x, "float32", 0.5, "POS", 0, want=2 * T + 9)
    assert exp[3] == f64bits(2 * T + 10)                                               # the quotient is exactly 1
    check(torch, dev, x, "float32", 0.5, "NEG", 0, want=None)
    x[2 * T + 11] = 0.75
    check(torch, dev, x, "float32", 0.5, "NEG", 0, want=2 * T + 11)
    inf = np.zeros((n, 2), np.float32)
    inf[70] = [np.inf, np.nan]                                                         # hypotf: inf wins over NaN
    check(torch, dev, inf, "complex_float32", 1e30, "POS", 0, want=69)


@pytest.mark.parametrize("dtype", ["int64", "uint64", "float64", "complex_int64"])
def test_search_values_that_round_across_the_level(torch, dev, dtype):
    """2^24 + 1 becomes 2^24 as a float, 2^24 + 3 becomes 2^24 + 4: the pair crosses 2^24 + 0.5 only after the conversion"""
    T, (n, _) = sizes(dev)
    x = np.zeros((n, 2) if M.is_complex(dtype) else n, M.np_scalar(dtype))
    at = T + 63
    if M.is_complex(dtype):
        x[at], x[at + 1], x[at + 2] = [16777217, 0], [16777219, 0], [16777219, 0]
    else:
        x[at:at + 3] = [16777217, 16777219, 16777219]
    check(torch, dev, x, dtype, 16777216.5, "POS", at, want=at)
    check(torch, dev, x, dtype, 16777216.5, "POS", 0, want=at)
    if not M.is_complex(dtype):
        big = np.zeros(n, M.np_scalar(dtype))
        big[100:103] = [2 ** 53 + 1, 2 ** 53 + 3, 0] if dtype != "float64" else [1.0 + 2.0 ** -30, 1.0 + 2.0 ** -22, 0.0]
        check(torch, dev, big, dtype, float(2 ** 53) + 2.0 if dtype != "float64" else 1.0 + 2.0 ** -24, "LEVEL", 0)


@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_search_every_type(torch, dev, dtype):
    T, _ = sizes(dev)
    case = M.Case("t", [dtype], [], [1], n=T + 333, seed=7)
    x = M.make_stream(case, 0)
    sc = M.np_scalar(dtype)
    level = (0.3 if sc.kind == "f" else 150.5 if sc.kind == "u" else 30.0) * (2.0 if M.is_complex(dtype) else 1.0)
    found = 0
    for slope in ("POS", "NEG", "LEVEL"):
        for start in (0, 100, T - 20):
            found += check(torch, dev, x, dtype, level, slope, start) is not None
    assert found == 9


@pytest.mark.parametrize("offset", [1, 3, 7])
def test_search_at_an_odd_byte_address(torch, dev, offset):
    T, _ = sizes(dev)
    for dtype in ("float32", "complex_int16", "float64", "uint8"):
        x = M.make_stream(M.Case("t", [dtype], [], [1], n=2 * T + 77, seed=3), 0)
        sc = M.np_scalar(dtype)
        level = 0.3 if sc.kind == "f" else 150.5 if sc.kind == "u" else 60.0
        assert check(torch, dev, x, dtype, level, "POS", T - 5, offset=offset) is not None


def test_search_host_memory(dev):
    """pageable host memory is staged; the result is the same"""
    T, _ = sizes(dev)
    x = M.make_stream(M.Case("t", ["int16"], [], [1], n=T + 50, seed=5), 0)
    t = dev.Trigger("int16", 20.0, "NEG")
    assert as_bits(t.search(x, 9)) == expected(x, "int16", 20.0, "NEG", 9)
    assert t.search(x[:1]) is None and t.search(x, len(x) - 1) is None


# ---- the capture
@pytest.mark.parametrize("elem_bytes", [[4], [2, 16, 3]])
@pytest.mark.parametrize("nev", [1, 5])
def test_capture_bytes(torch, dev, elem_bytes, nev):
    rng = np.random.default_rng(11)
    t = dev.Trigger("uint8")
    for W in (37, 1500):                                                                # a row inside one chunk of a workgroup, and one over several
        n = 4 * W + 100
        starts = np.sort(rng.integers(0, n - W, nev)).astype(np.uint64)
        starts[-1] = n - W                                                              # the last row ends with the buffer
        srcs = [rng.integers(0, 256, n * eb).astype(np.uint8) for eb in elem_bytes]
        want = [np.stack([s[int(a) * eb:(int(a) + W) * eb] for a in starts]) for s, eb in zip(srcs, elem_bytes)]
        # device memory at odd addresses, through the host-pointer call and through the device call
        ins = [to_device(torch, s, 1 + 2 * p) for p, s in enumerate(srcs)]
        outs = [to_device(torch, np.full(nev * W * eb, CANARY, np.uint8), 3 + p, tail=64) for p, eb in enumerate(elem_bytes)]
        t.capture([a for _, a in ins], elem_bytes, starts, W, outs=[a for _, a in outs])
        torch.cuda.synchronize()
        for (buf, _), w, p in zip(outs, want, range(len(want))):
            raw = buf.cpu().numpy()
            assert (raw[3 + p:3 + p + w.size] == w.reshape(-1)).all()
            assert (raw[:3 + p] == CANARY).all() and (raw[3 + p + w.size:] == CANARY).all()
        outs2 = [to_device(torch, np.full(nev * W * eb, CANARY, np.uint8), 5, tail=64) for eb in elem_bytes]
        dstarts = torch.from_numpy(starts.view(np.int64).copy()).cuda()
        t.capture_dev([a for _, a in ins], elem_bytes, dstarts, nev, W, [a for _, a in outs2])
        torch.cuda.synchronize()
        for (buf, _), w in zip(outs2, want):
            raw = buf.cpu().numpy()
            assert (raw[5:5 + w.size] == w.reshape(-1)).all() and (raw[:5] == CANARY).all() and (raw[5 + w.size:] == CANARY).all()
        # pageable host memory both ways
        got = t.capture(srcs, elem_bytes, starts, W)
        for g, w in zip(got, want):
            assert (g == w).all()


# ---- the block: the recorded cases on buffers in device memory
@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_block_equals_the_recorded_reference(torch, blocks, golden, case):
    streams, ref = golden[case.name]
    blk = blocks.make("/comms/wave_trigger", None, module="trigger")
    if len(case.dtypes) > 1:
        blk.call("setNumPorts", len(case.dtypes))
    held = [to_device(torch, s, 0) for s in streams]
    got = M.flatten(M.run_calls(case, streams, M.block_work(blk, streams, [a for _, a in held], blocks.Label), M.block_call(blk), blk.activate))
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (case.name, k)
    blk.close()


def test_block_on_page_locked_and_pageable_buffers(blocks, golden):
    """the same calls wherever the port buffers lie: the block's own page-locked slab, and pageable memory"""
    case = [c for c in M.CASES if c.name == "two_ports_aligned"][0]
    streams, ref = golden[case.name]
    blk = blocks.make("/comms/wave_trigger", None, module="trigger")
    blk.call("setNumPorts", 2)
    blk.call("setPortSlabBytes", 64 << 10)
    slabs = []
    for s in streams:
        arr, pinned = blk.port_buffer(0, (s.nbytes,), np.uint8)
        assert pinned
        arr[:] = s.view(np.uint8).reshape(-1)
        slabs.append(arr)
    got = M.flatten(M.run_calls(case, streams, M.block_work(blk, streams, [a.ctypes.data for a in slabs], blocks.Label), M.block_call(blk), blk.activate))
    assert got == ref
    blk2 = blocks.make("/comms/wave_trigger", None, module="trigger")
    blk2.call("setNumPorts", 2)
    got = M.flatten(M.run_calls(case, streams, M.block_work(blk2, streams, [s.ctypes.data for s in streams], blocks.Label), M.block_call(blk2), blk2.activate))
    assert got == ref
