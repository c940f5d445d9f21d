"""GPU suite of /comms/bits_to_symbols, /comms/symbols_to_bits, /comms/bytes_to_symbols and /comms/symbols_to_bytes (pcx_repack_*,
device.SymbolRepacker and the blocks of libpcx_repack_blocks.so).

Everything is held by exact equality: to the recorded reference outputs (tests/golden/repack.npz) and to the numpy model
(tests/repack_model.py), which the CPU suite holds to the same recording.  Inputs are full-range bytes throughout, so the unmasked
pack of symbols_to_bytes, the != 0 test of bits_to_symbols and the low-bits-only reading of symbols_to_bits are all exercised."""
import os

import numpy as np
import pytest

import repack_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "repack.npz"))


def _torch_of(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.uint8, device="cuda:0")


def pieces(n, cuts):
    """[(start, count)] covering n elements: the cuts, then the rest"""
    out, pos = [], 0
    for c in cuts:
        c = min(c, n - pos)
        if c > 0:
            out.append((pos, c))
            pos += c
    if pos < n:
        out.append((pos, n - pos))
    return out


def on_device(r, x):
    """one process_dev call over the host array x"""
    xd, yd = _torch_of(x), _zeros(max(1, r.out_elems(x.size)))
    r.process_dev(xd, yd, x.size)
    return yd.cpu().numpy()[:r.out_elems(x.size)]


# ---- the recorded cases
@pytest.mark.parametrize("device_pointers", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("whole", [False, True], ids=["cut", "whole"])
def test_every_fixture_case_through_the_c_abi(dev, golden, whole, device_pointers):
    for name in M.CASES:
        kind, order, w = name.split("/")
        w = int(w)
        r = dev.SymbolRepacker(kind, w, order)
        gin, gout = r.group()
        inputs = [("in_full", "out/")]
        if kind in ("bits_to_symbols", "symbols_to_bits"):
            inputs.append(("in_bits", "out_bits/"))
        for src, dst in inputs:
            x = golden[src]
            cuts = [] if whole else [gin, 5 * gin, 37 * gin]
            if device_pointers:
                xd, yd = _torch_of(x), _zeros(r.out_elems(x.size))
                for a, c in pieces(x.size, cuts):
                    r.process_dev(xd[a:a + c], yd[a // gin * gout:], c)
                got = yd.cpu().numpy()
            else:
                got = np.concatenate([r.process(x[a:a + c]) for a, c in pieces(x.size, cuts)])
            assert np.array_equal(got, golden[dst + name]), (name, src)
        if kind == "symbols_to_bytes":
            x = golden["in_full"] & np.uint8((1 << w) - 1)
            got = on_device(r, x) if device_pointers else r.process(x)
            assert np.array_equal(got, golden["out_masked/" + name]), name
        r.close()


# ---- seams of the tiling
@pytest.mark.parametrize("kind", M.KINDS)
def test_lengths_around_the_tile_equal_the_model(dev, kind):
    rng = np.random.default_rng(41)
    for w in (1, 3, 5, 6, 7, 8):
        for order in M.ORDERS:
            r = dev.SymbolRepacker(kind, w, order)
            (tile, _), (gin, _) = r.geometry(), r.group()
            assert tile % gin == 0
            x = rng.integers(0, 256, 3 * tile + gin, dtype=np.uint8)
            want = M.convert(kind, x, w, order)
            for n in (gin, tile - gin, tile, tile + gin, 3 * tile + gin):
                got = on_device(r, x[:n])
                assert np.array_equal(got, want[:r.out_elems(n)]), (kind, w, order, n)
            r.close()


@pytest.mark.parametrize("kind", M.KINDS)
def test_any_alignment_of_either_pointer_and_nothing_written_outside(dev, kind):
    import torch
    rng = np.random.default_rng(42)
    guard = 64
    for w, order in ((3, "MSBit"), (3, "LSBit"), (8, "MSBit")):
        r = dev.SymbolRepacker(kind, w, order)
        (tile, _), (gin, _) = r.geometry(), r.group()
        for n in (3 * tile + gin, gin):
            x = rng.integers(0, 256, n, dtype=np.uint8)
            want = M.convert(kind, x, w, order)
            m = want.size
            xd = _torch_of(x)
            for in_off in (1, 3, 8, 15):
                xin = _zeros(n + 16)
                xin[in_off:in_off + n].copy_(xd)
                for out_off in (1, 3, 8, 15):
                    yd = torch.full((guard + 16 + m + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
                    assert (xin.data_ptr() + in_off) % 16 == in_off and (yd.data_ptr() + guard + out_off) % 16 == out_off
                    r.process_dev(xin[in_off:], yd[guard + out_off:], n)
                    got = yd.cpu().numpy()
                    at = guard + out_off
                    assert np.array_equal(got[at:at + m], want), (kind, w, order, n, in_off, out_off)
                    assert (got[:at] == 0xA5).all() and (got[at + m:] == 0xA5).all(), (kind, w, order, n, in_off, out_off)
        r.close()


def windows_equal_the_model(r, kind, w, order, xd, yd, windows):
    gin, gout = r.group()
    for a, b in windows:
        assert a % gin == 0 and b % gin == 0 and a < b, (a, b, gin)
        want = M.convert(kind, xd[a:b].cpu().numpy(), w, order)
        got = yd[a // gin * gout:b // gin * gout].cpu().numpy()
        assert np.array_equal(got, want), (kind, w, order, a, b)


@pytest.mark.parametrize("kind", M.KINDS)
def test_a_call_longer_than_one_slice(dev, kind):
    import torch
    for w, order in ((7, "MSBit"), (2, "LSBit")):
        r = dev.SymbolRepacker(kind, w, order)
        (tile, slc), (gin, _) = r.geometry(), r.group()
        assert slc <= 64 << 20 and slc % tile == 0
        n = slc + gin
        xd = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0")
        yd = _zeros(r.out_elems(n))
        r.process_dev(xd, yd, n)
        windows_equal_the_model(r, kind, w, order, xd, yd, [(0, 2 * tile), (slc - 2 * tile, n), (n - gin, n), (slc // tile // 2 * tile, slc // tile // 2 * tile + tile)])
        del xd, yd
        r.close()
    torch.cuda.empty_cache()


def test_a_call_beyond_2_32_elements(dev):
    import torch
    kind, w, order = "symbols_to_bytes", 1, "MSBit"
    r = dev.SymbolRepacker(kind, w, order)
    tile, slc = r.geometry()
    n = (1 << 32) + 8 * tile
    xd = torch.randint(-(1 << 63), (1 << 63) - 1, (n // 8,), dtype=torch.int64, device="cuda:0").view(torch.uint8)
    assert xd.numel() == n
    yd = _zeros(r.out_elems(n))
    r.process_dev(xd, yd, n)
    edge = 1 << 32
    windows_equal_the_model(r, kind, w, order, xd, yd, [(0, tile), (edge - 2 * tile, edge + 2 * tile), (n - 2 * tile, n), (edge // slc * slc - tile, edge // slc * slc + tile)])
    del xd, yd
    r.close()
    torch.cuda.empty_cache()


# ---- graphs
def test_captured_graph_of_an_expanding_and_a_contracting_kind_replays_exact(dev):
    import torch
    w, order = 5, "MSBit"
    up, down = dev.SymbolRepacker("bytes_to_symbols", w, order), dev.SymbolRepacker("symbols_to_bytes", w, order)
    tile, _ = up.geometry()
    n = 3 * tile + 5 * 7
    rng = np.random.default_rng(43)
    xd, sym, back = _zeros(n), _zeros(up.out_elems(n)), _zeros(n)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def chain():
        up.process_dev(xd, sym, n, stream=s)
        down.process_dev(sym, back, sym.numel(), stream=s)
    with torch.cuda.stream(s):
        chain()                                                  # the first calls, outside the graph: the stream is bound
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for _ in range(2):
        x = rng.integers(0, 256, n, dtype=np.uint8)
        xd.copy_(_torch_of(x))
        sym.zero_()
        back.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(sym.cpu().numpy(), M.convert("bytes_to_symbols", x, w, order))
        assert np.array_equal(back.cpu().numpy(), x)
    up.close()
    down.close()


# ---- the blocks
def test_blocks_follow_the_reference_arithmetic_and_adjust_labels(dev):
    from pothoscomms_amd import blocks as B
    rng = np.random.default_rng(44)
    for prefix in ("/comms/", "/blocks/"):
        for kind in M.KINDS:
            for w, order in ((3, "MSBit"), (6, "LSBit")):
                b = B.make(prefix + kind, module="repack")
                b.call("setModulus", w)
                b.call("setBitOrder", order)
                gin, gout = M.group(kind, w)
                mult, div = M.label_ratio(kind, w)
                # the input is not a whole number of groups (where a group is more than one element); the output has room
                x = rng.integers(0, 256, 37 * gin + (gin - 1), dtype=np.uint8)
                labels = [B.Label("a", 0), B.Label("b", gin, data=7, width=gin), B.Label("c", 37 * gin - 1), B.Label("late", 37 * gin)]
                y, consumed, produced, reserve, posted = b.work(x, 40 * gout + 1, labels=labels)
                assert (consumed, produced, reserve) == M.work_sizes(kind, w, x.size, 40 * gout + 1) + (M.reserve(kind, w),)
                assert (consumed, produced) == (37 * gin, 37 * gout)
                assert np.array_equal(y, M.convert(kind, x[:consumed], w, order)), (kind, w, order)
                assert posted == [B.Label("a", 0, width=1 * mult // div), B.Label("b", gin * mult // div, data=7, width=gin * mult // div),
                                  B.Label("c", (37 * gin - 1) * mult // div, width=1 * mult // div)], (kind, w, posted)
                # the output space is the limit, and is rounded down to whole groups too
                room = 5 * gout + (gout - 1)
                y, consumed, produced, reserve, _ = b.work(x, room)
                assert (consumed, produced, reserve) == (5 * gin, 5 * gout, M.reserve(kind, w)), (kind, w)
                assert np.array_equal(y, M.convert(kind, x[:consumed], w, order)), (kind, w, order)
                b.close()


# ---- round trips (what smoke() runs)
def test_the_two_chains_of_smoke_return_their_input(dev):
    rng = np.random.default_rng(45)
    payload = rng.integers(0, 256, 40000, dtype=np.uint8)
    qpsk = np.array([[-1, -1], [-1, 1], [1, 1], [1, -1]], np.float32)
    sym = dev.SymbolRepacker("bytes_to_symbols", 2, "MSBit").process(payload)
    assert np.array_equal(sym, M.convert("bytes_to_symbols", payload, 2, "MSBit"))
    sliced = dev.SymbolSlicer("complex_float32", qpsk).process(dev.SymbolMapper("complex_float32", qpsk).process(sym))
    assert np.array_equal(dev.SymbolRepacker("symbols_to_bytes", 2, "MSBit").process(sliced), payload)
    bits = dev.SymbolRepacker("symbols_to_bits", 8).process(payload)
    assert bits.size == 8 * payload.size and bits.max() == 1
    for mode in ("additive", "multiplicative"):
        scrambled = dev.Scrambler(False, mode, 0x11021, 0xACE1).process(bits)
        assert not np.array_equal(scrambled, bits)
        clear = dev.Scrambler(True, mode, 0x11021, 0xACE1).process(scrambled)
        assert np.array_equal(dev.SymbolRepacker("bits_to_symbols", 8).process(clear), payload), mode
