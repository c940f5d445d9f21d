"""GPU suite of /comms/scrambler and /comms/descrambler (pcx_scrambler_*, device.Scrambler, the blocks in libpcx_digital_blocks.so).

Everything is held by exact equality: to the recorded reference outputs (tests/golden/scrambler.npz), to the bit-serial model
(tests/scrambler_model.py), and for streams too long for it to the model's first 8192 bits plus the window check of every later
bit -- under SCAN the state in front of bit i is a function of the m pairs before it, so the two prove the stream by induction."""
import os

import numpy as np
import pytest

import scrambler_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT63 = 0x8000000000000003
# kind -> (descramble, mode)
KINDS = {"additive": (False, "additive"), "scrambler": (False, "multiplicative"), "descrambler": (True, "multiplicative")}
LONG_POLYS = [(0x19, 4, 0x9), (0x11021, 16, 0xACE1), (BIT63, 63, 0x1234567)]      # polynomial, m, seed


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "scrambler.npz"))


def _torch_of(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def merged(ops):
    """the calls of a case with neighbouring work() calls joined: the stream whole, as far as the setters in it allow"""
    out = []
    for op, v in ops:
        if op == "work" and out and out[-1][0] == "work":
            out[-1] = ("work", out[-1][1] + v)
        else:
            out.append((op, v))
    return out


def replay(h, ops, x, on_device):
    """the calls of a fixture case on a device.Scrambler; returns (outputs, plan at the first work())"""
    import torch
    outs, pos, plan = [], 0, None
    xd = _torch_of(x) if on_device else None
    for op, v in ops:
        if op == "work":
            if plan is None:
                plan = h.plan()
            if on_device:
                y = torch.empty(v, dtype=torch.uint8, device="cuda:0")
                h.process_dev(xd[pos:pos + v], y, v)
                outs.append(y.cpu().numpy())
            else:
                outs.append(h.process(x[pos:pos + v]))
            pos += v
        else:
            getattr(h, "set_" + op)(v)
    return np.concatenate(outs), plan


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("whole", [False, True], ids=["cut", "whole"])
def test_every_fixture_case_through_the_c_abi(dev, golden, whole, on_device):
    from pothoscomms_amd import _lib
    x = golden["in"]
    for key in golden["cases"]:
        cfg = golden["cfg/" + key]
        ops = M.case_ops(cfg, golden["cuts"])
        h = dev.Scrambler(descramble=bool(cfg[0]))
        got, plan = replay(h, merged(ops) if whole else ops, x, on_device)
        assert plan == (_lib.SCR_SERIAL if cfg[6] else _lib.SCR_SCAN), key
        assert np.array_equal(got, np.unpackbits(golden["out/" + key])[:x.shape[0]]), key
        assert h.state() == tuple(int(v) for v in golden["state/" + key]), key
        assert (h.poly(), h.seed()) == (int(cfg[4]), int(cfg[5])) and h.mode() == ("multiplicative" if cfg[1] else "additive")


def test_every_fixture_case_through_the_blocks(dev, golden):
    from pothoscomms_amd import blocks as B
    x = golden["in"]
    for key in golden["cases"]:
        cfg = golden["cfg/" + key]
        name = "descrambler" if cfg[0] else "scrambler"
        for path in ("/comms/" + name, "/blocks/" + name):
            blk = B.make(path, module="digital")
            assert (blk.in_dtype, blk.out_dtype) == ("uint8", "uint8")
            assert (blk.call("mode"), blk.call("poly"), blk.call("seed"), blk.call("sync")) == ("multiplicative", 0x19, 1, "")
            blk.activate()
            outs, pos = [], 0
            for op, v in M.case_ops(cfg, golden["cuts"]):
                if op == "work":
                    y, consumed, produced, _, _ = blk.work(x[pos:pos + v], v + 5)        # min(in, out) elements
                    assert consumed == produced == v
                    outs.append(y[:produced].copy())
                    pos += v
                else:
                    blk.call({"mode": "setMode", "poly": "setPoly", "seed": "setSeed"}[op], v)
            assert np.array_equal(np.concatenate(outs), np.unpackbits(golden["out/" + key])[:x.shape[0]]), (key, path)
            assert (blk.call("poly"), blk.call("seed")) == (int(cfg[4]), int(cfg[5]))
            blk.close()


def test_block_exceptions_and_set_device_starts_the_register_over(dev):
    from pothoscomms_amd import _lib, blocks as B
    x = np.random.default_rng(5).integers(0, 256, 5000, dtype=np.uint8)
    for name, descramble in (("scrambler", False), ("descrambler", True)):
        blk = B.make("/comms/" + name, module="digital")
        with pytest.raises(_lib.InvalidArgument, match="unknown mode: xor"):
            blk.call("setMode", "xor")
        assert blk.call("mode") == "multiplicative"
        blk.call("setSync", "0110" * 16)
        assert blk.call("sync") == "0110" * 16
        for word, why in (("01" * 33, "sync word max len 64 bits"), ("01x1", "sync word must be 0s and 1s")):
            with pytest.raises(_lib.PcxError, match=why) as e:
                blk.call("setSync", word)
            assert not isinstance(e.value, _lib.InvalidArgument)            # a RangeException, not an InvalidArgumentException
        blk.call("setMode", "additive")
        blk.call("setPoly", 0x11021)
        blk.call("setSeed", 0xACE1)
        first, _, p1, _, _ = blk.work(x, 5000)
        again, _, _, _, _ = blk.work(x, 5000)
        assert not np.array_equal(first, again)                             # the register ran on
        blk.call("setDevice", 0)
        assert blk.call("getDevice") == 0 and (blk.call("mode"), blk.call("poly"), blk.call("seed")) == ("additive", 0x11021, 0xACE1)
        fresh, _, p2, _, _ = blk.work(x, 5000)
        assert p1 == p2 == 5000 and np.array_equal(first, fresh)
        assert np.array_equal(first, M.Model(descramble, "additive", 0x11021, 0xACE1).process(x))
        assert blk.call("getPortSlabBytes") == 64 << 20


@pytest.mark.parametrize("kind", list(KINDS))
def test_scan_equals_the_model_around_the_run_and_the_tile(dev, kind):
    """calls of run - 1, run, run + 1, tile - 1, tile, tile + 1 bits and odd ones between, the register carried; on the device the
    odd call lengths also leave the buffers off the 16-byte grid"""
    import torch
    from pothoscomms_amd import _lib
    run, tile, _, _ = dev.Scrambler.geometry()
    cuts = [run - 1, run, run + 1, 3, tile - 1, tile, tile + 1, 1, 2 * tile + run + 5, 64, 2 * run - 1, 7 * tile + 3 * run + 11]
    x = np.random.default_rng(6).integers(0, 256, sum(cuts), dtype=np.uint8)
    descramble, mode = KINDS[kind]
    for poly, m, seed in LONG_POLYS + [(0x7, 2, 1), (0x80000D, 23, 0x2A5A5A)]:
        model = M.Model(descramble, mode, poly, seed)
        want = model.process(x)
        for on_device in (False, True):
            h = dev.Scrambler(descramble, mode, poly, seed)
            assert h.plan() == _lib.SCR_SCAN
            xd, outs, pos = _torch_of(x), [], 0
            for c in cuts:
                if on_device:
                    y = torch.empty(c + 1, dtype=torch.uint8, device="cuda:0")[1:]          # off the grid as well
                    h.process_dev(xd[pos:pos + c], y, c)
                    outs.append(y.cpu().numpy())
                else:
                    outs.append(h.process(x[pos:pos + c]))
                pos += c
            assert np.array_equal(np.concatenate(outs), want), (kind, hex(poly), on_device)
            assert h.state() == (model.l.data, model.l.mask), (kind, hex(poly), on_device)


@pytest.mark.parametrize("kind", list(KINDS))
def test_scan_equals_the_model_around_the_carrys_run_of_tiles(dev, kind):
    import torch
    _, tile, group, _ = dev.Scrambler.geometry()
    cuts = [group - 1, group, group + 1]
    descramble, mode = KINDS[kind]
    x = np.random.default_rng(7).integers(0, 256, sum(cuts), dtype=np.uint8)
    model = M.Model(descramble, mode, 0x11021, 0xACE1)
    want = model.process(x)
    h = dev.Scrambler(descramble, mode, 0x11021, 0xACE1)
    xd, pos = _torch_of(x), 0
    yd = torch.empty_like(xd)
    for c in cuts:
        h.process_dev(xd[pos:pos + c], yd[pos:pos + c], c)
        pos += c
    got = yd.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (kind, int(bad[0]), bad.size)
    assert h.state() == (model.l.data, model.l.mask)


@pytest.mark.parametrize("poly, m, seed", LONG_POLYS, ids=["0x19", "0x11021", "bit63"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_64mi_bits_on_the_device(dev, kind, poly, m, seed):
    import torch
    from pothoscomms_amd import _lib
    n = 64 << 20
    descramble, mode = KINDS[kind]
    pol = M.u64(poly) | 1
    g = torch.Generator(device="cuda:0").manual_seed(8)
    x = torch.randint(0, 256, (n,), device="cuda:0", generator=g, dtype=torch.uint8)
    y = torch.empty_like(x)
    h = dev.Scrambler(descramble, mode, poly, seed)
    assert h.plan() == _lib.SCR_SCAN
    h.process_dev(x, y, n)
    head = M.Model(descramble, mode, poly, seed).process(x[:8192].cpu().numpy())
    assert np.array_equal(y[:8192].cpu().numpy(), head)
    assert int(y.max().item()) <= 1
    assert M.window_check(x, y, pol, m, kind) == 0
    data, mask = h.state()
    assert data == M.state_from_tail(x, y, pol, m, kind) and mask == M.glfsr_init(M.Lfsr(), poly, seed).mask
    if kind == "additive":
        assert data == M.jump(seed, n, pol, m)
    if kind == "scrambler":
        back = torch.empty_like(x)
        dev.Scrambler(True, mode, poly, seed).process_dev(y, back, n)
        assert torch.equal(back, x & 1)


def test_beyond_2_32_bits_additive(dev):
    import torch
    n = (1 << 32) + 12345
    free, _ = torch.cuda.mem_get_info()
    if free < 2 * n + (3 << 30):
        pytest.skip("needs %d bytes of device memory" % (2 * n + (3 << 30)))
    _, _, _, slc = dev.Scrambler.geometry()
    poly, m, seed = 0x11021, 16, 0xACE1
    x = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(9)
    for a in range(0, n, 1 << 30):
        b = min(n, a + (1 << 30))
        x[a:b] = torch.randint(0, 256, (b - a,), device="cuda:0", generator=g, dtype=torch.uint8)
    y = torch.empty_like(x)
    h = dev.Scrambler(False, "additive", poly, seed)
    h.process_dev(x, y, n)
    torch.cuda.synchronize()
    # at every slice seam: 64 bits on either side against the model started from the register jumped there
    for s in list(range(0, n, slc)) + [n - 64]:
        a, b = max(0, s - 64), min(n, s + 64)
        model = M.Model(False, "additive", poly, seed)
        model.l.data = M.jump(seed, a, poly, m)
        assert np.array_equal(y[a:b].cpu().numpy(), model.process(x[a:b].cpu().numpy())), s
    assert h.state()[0] == M.jump(seed, n, poly, m)
    assert M.window_check(x, y, poly, m, "additive") == 0


@pytest.mark.parametrize("kind", list(KINDS))
def test_upper_bits_of_the_input_bytes_do_not_count(dev, kind):
    descramble, mode = KINDS[kind]
    x = np.random.default_rng(10).integers(0, 256, 100000, dtype=np.uint8)
    assert x.max() > 1
    a = dev.Scrambler(descramble, mode, 0x11021, 0xACE1).process(x)
    b = dev.Scrambler(descramble, mode, 0x11021, 0xACE1).process(x & 1)
    assert np.array_equal(a, b) and a.max() == 1


@pytest.mark.parametrize("kind", list(KINDS))
def test_in_place_is_supported_and_other_overlap_refused(dev, kind):
    import torch
    from pothoscomms_amd import _lib
    descramble, mode = KINDS[kind]
    n = 300000
    x = np.random.default_rng(11).integers(0, 256, n + 16, dtype=np.uint8)
    for off in (0, 3):                                        # on and off the 16-byte grid
        want = dev.Scrambler(descramble, mode, BIT63, 0x1234567).process(x[off:off + n])
        xd = _torch_of(x)
        dev.Scrambler(descramble, mode, BIT63, 0x1234567).process_dev(xd[off:off + n], xd[off:off + n], n)
        assert np.array_equal(xd[off:off + n].cpu().numpy(), want)
        assert np.array_equal(xd[off + n:].cpu().numpy(), x[off + n:]) and np.array_equal(xd[:off].cpu().numpy(), x[:off])
    h = dev.Scrambler(descramble, mode)
    xd = _torch_of(x)
    with pytest.raises(_lib.InvalidArgument, match="overlaps"):
        h.process_dev(xd[:1000], xd[1:1001], 1000)
    with pytest.raises(_lib.InvalidArgument, match="overlaps"):
        h.process_dev(xd[8:1008], xd[:1000], 1000)


@pytest.mark.parametrize("kind", list(KINDS))
def test_graph_capture_replays_bit_equal(dev, kind):
    import torch
    descramble, mode = KINDS[kind]
    n = 1 << 20
    x = np.random.default_rng(12).integers(0, 256, 4 * n, dtype=np.uint8)
    ref = dev.Scrambler(descramble, mode, 0x11021, 0xACE1)
    ref.process(x[:n])
    h = dev.Scrambler(descramble, mode, 0x11021, 0xACE1)
    xd = _torch_of(x)
    yd = torch.empty_like(xd)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        h.process_dev(xd[:n], yd[:n], n, stream=s)           # the first call, outside the graph: the stream is bound
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for k in range(1, 4):
            h.process_dev(xd[k * n:(k + 1) * n], yd[k * n:(k + 1) * n], n, stream=s)
    for _ in range(2):                                        # every replay carries the register on from the one before
        want = np.concatenate([ref.process(x[k * n:(k + 1) * n]) for k in range(1, 4)])
        yd.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(yd[n:].cpu().numpy(), want)
    assert h.state() == ref.state()


def test_serial_at_64_ki_bits_equals_the_model(dev):
    from pothoscomms_amd import _lib
    x = np.random.default_rng(13).integers(0, 256, 64 << 10, dtype=np.uint8)
    for descramble, mode in KINDS.values():
        for poly, seed in ((0x19, 0xF3), (0x19, -1), (0x11021, 1 << 16)):
            h = dev.Scrambler(descramble, mode, poly, seed)
            assert h.plan() == _lib.SCR_SERIAL
            model = M.Model(descramble, mode, poly, seed)
            cuts = [1, 4095, 30000, x.shape[0] - 34096]
            got = np.concatenate([h.process(x[a:a + c]) for a, c in zip(np.cumsum([0] + cuts[:-1]), cuts)])
            assert np.array_equal(got, model.process(x)), (descramble, mode, hex(poly), seed)
            assert h.state() == (model.l.data, model.l.mask)


def test_set_poly_and_set_seed_mid_stream_start_over_and_set_mode_does_not(dev):
    x = np.random.default_rng(14).integers(0, 256, 50000, dtype=np.uint8)
    h = dev.Scrambler(False, "multiplicative", 0x11021, 0xACE1)
    model = M.Model(False, "multiplicative", 0x11021, 0xACE1)
    assert np.array_equal(h.process(x[:20000]), model.process(x[:20000]))
    h.set_mode("additive")
    model.set_mode("additive")
    assert np.array_equal(h.process(x[20000:30000]), model.process(x[20000:30000]))
    assert h.state() == (model.l.data, model.l.mask)
    h.set_seed(0x77)
    model.set_seed(0x77)
    assert h.state() == (0x77, model.l.mask)
    assert np.array_equal(h.process(x[30000:40000]), model.process(x[30000:40000]))
    h.set_poly(0x19)                      # the seed 0x77 is above 2^4 now: SERIAL
    model.set_poly(0x19)
    from pothoscomms_amd import _lib
    assert h.plan() == _lib.SCR_SERIAL and model.plan() == "SERIAL"
    assert np.array_equal(h.process(x[40000:]), model.process(x[40000:]))
    assert h.state() == (model.l.data, model.l.mask)
