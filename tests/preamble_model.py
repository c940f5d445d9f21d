"""Model of /comms/preamble_correlator (the reference's digital/PreambleCorrelator.cpp), the yardstick of tests/test_preamble_*.py.

The plain restatement of the reference's loop below (`distances_plain`, `matches_plain`) is held to tests/golden/preamble.npz, what the
reference's own work() posted when compiled against a stand-in framework (tests/golden/make_preamble_golden.py; `golden_cases` unpacks
it), and is the yardstick wherever no recording reaches.  Three parts:

  1. the reference's loop as it stands (PreambleCorrelator.cpp:134-151): for every position n < len(x) - P,
     dist = sum over i < P of popcount(preamble[i] ^ x[n + i]) through a 256-entry popcount table, O(N P), and a label at n + P
     wherever dist <= threshold;
  2. a second formulation written independently of it: per bit plane of the symbols, a plane in which the preamble is all zero
     contributes a difference of prefix sums, any other plane 32-symbol windows packed into words, XORed with the packed preamble
     and counted through a 16-bit table (`distances_planes`);
  3. the second formulation on torch tensors, in chunks of positions, on whatever device the tensors are on (`torch_distances`,
     `torch_check`): what checks a 64 Mi-symbol call on the GPU.
"""
import numpy as np

POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint32)


def _u8(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8).reshape(-1))
    return a


def positions(n_in, P):
    """work() consumes and forwards n_in - P elements when n_in > P, nothing otherwise (:123-128)"""
    return n_in - P if n_in > P else 0


# ---- 1. the reference's loop
def distances_plain(preamble, x):
    pre, x = _u8(preamble), _u8(x)
    if pre.size == 0:
        raise ValueError("preamble cannot be empty")
    N = positions(x.size, pre.size)
    d = np.zeros(N, np.uint32)
    for i in range(pre.size):
        d += POP8[x[i:i + N] ^ pre[i]]
    return d


def matches_of(dist, threshold, P):
    """label indices n + P (uint64, ascending) of the positions with dist <= threshold: not clamped to the forwarded elements"""
    return (np.nonzero(dist <= threshold)[0] + P).astype(np.uint64)


def matches_plain(preamble, threshold, x):
    """(label indices, n_positions, n_matches)"""
    d = distances_plain(preamble, x)
    idx = matches_of(d, threshold, _u8(preamble).size)
    return idx, d.size, idx.size


# ---- 2. per bit plane: prefix sums and packed words
POP16 = (POP8[np.arange(65536) & 0xFF] + POP8[np.arange(65536) >> 8]).astype(np.uint32)


def pack_preamble(preamble):
    """(active plane mask, words[8][K]): bit i of words[b][k] = bit b of preamble[32 k + i]"""
    pre = _u8(preamble)
    K = (pre.size + 31) // 32
    words = np.zeros((8, K), np.uint64)
    for b in range(8):
        bits = ((pre >> b) & 1).astype(np.uint64)
        for i in np.nonzero(bits)[0]:
            words[b, i // 32] |= np.uint64(1) << np.uint64(i % 32)
    active = 0
    for b in range(8):
        if words[b].any():
            active |= 1 << b
    return active, words


def distances_planes(preamble, x):
    pre, x = _u8(preamble), _u8(x)
    P = pre.size
    N = positions(x.size, P)
    d = np.zeros(N, np.uint64)
    if N == 0:
        return d.astype(np.uint32)
    active, words = pack_preamble(pre)
    K = (P + 31) // 32
    for b in range(8):
        plane = ((x >> b) & 1).astype(np.uint64)
        if not (active >> b) & 1:
            pref = np.concatenate([[0], np.cumsum(plane)]).astype(np.uint64)
            d += pref[P:P + N] - pref[:N]
            continue
        padded = np.concatenate([plane, np.zeros(32 * K + 32, np.uint64)])
        win = np.zeros(N + 32 * K, np.uint64)                 # win[j]: the 32 plane bits from position j on, bit i = position j + i
        for i in range(32):
            win |= padded[i:i + win.size] << np.uint64(i)
        for k in range(K):
            left = P - 32 * k
            keep = np.uint64(0xFFFFFFFF if left >= 32 else (1 << left) - 1)
            v = (win[32 * k:32 * k + N] ^ words[b, k]) & keep
            d += POP16[(v & np.uint64(0xFFFF)).astype(np.int64)] + POP16[(v >> np.uint64(16)).astype(np.int64)]
    return d.astype(np.uint32)


def matches_planes(preamble, threshold, x):
    d = distances_planes(preamble, x)
    idx = matches_of(d, threshold, _u8(preamble).size)
    return idx, d.size, idx.size


# ---- 3. the same on torch tensors, in chunks
def torch_distances(preamble, x, start, stop):
    """distances of the positions [start, stop) of the uint8 tensor x as an int64 tensor on x's device; stop <= len(x) - P"""
    import torch
    pre = _u8(preamble)
    P = pre.size
    n = stop - start
    dev = x.device
    active, words = pack_preamble(pre)
    K = (P + 31) // 32
    seg = x[start:stop + P].to(torch.int64)
    pop16 = torch.from_numpy(POP16.astype(np.int64)).to(dev)
    d = torch.zeros(n, dtype=torch.int64, device=dev)
    for b in range(8):
        plane = (seg >> b) & 1
        if not (active >> b) & 1:
            pref = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(plane, 0)])
            d += pref[P:P + n] - pref[:n]
            continue
        padded = torch.cat([plane, torch.zeros(32 * K + 32 - P + 1, dtype=torch.int64, device=dev)])
        size = n + 32 * K - 32 + 1
        win = torch.zeros(size, dtype=torch.int64, device=dev)
        for i in range(32):
            win |= padded[i:i + size] << i
        for k in range(K):
            left = P - 32 * k
            keep = 0xFFFFFFFF if left >= 32 else (1 << left) - 1
            v = (win[32 * k:32 * k + n] ^ int(words[b, k])) & keep
            d += pop16[v & 0xFFFF] + pop16[v >> 16]
    return d


def torch_check(preamble, threshold, x, dist=None, idx=None, chunk=1 << 22):
    """Walks the positions of the uint8 tensor x in chunks.  Returns (n_positions, n_matches, wrong distances, wrong indices): dist (a
    tensor of n_positions distances) and idx (a tensor of the label indices, complete and ascending) are compared where given."""
    import torch
    P = _u8(preamble).size
    N = positions(x.numel(), P)
    bad_d = bad_i = nm = 0
    for a in range(0, N, chunk):
        b = min(N, a + chunk)
        d = torch_distances(preamble, x, a, b)
        if dist is not None:
            bad_d += int((dist[a:b].to(torch.int64) != d).sum())
        hit = torch.nonzero(d <= threshold).reshape(-1) + (a + P)
        if idx is not None:
            got = idx[nm:nm + hit.numel()].to(torch.int64)
            bad_i += hit.numel() - got.numel() if got.numel() != hit.numel() else int((got != hit).sum())
        nm += int(hit.numel())
    if idx is not None and idx.numel() != nm:
        bad_i += abs(int(idx.numel()) - nm)
    return N, nm, bad_d, bad_i


# ---- streams and the block's work() loop
def plant(x, preamble, at):
    """x with the preamble written at every offset of `at`"""
    x = x.copy()
    pre = _u8(preamble)
    for a in at:
        x[a:a + pre.size] = pre
    return x


def golden_stream(base, width, n, fill, mask, flip_at, flip_xor, preamble, at):
    """a stream of tests/golden/preamble.npz: n symbols of the base array of that width (width 0: n times `fill`), the preamble planted at
    `at`, then one symbol xor-ed where flip_at >= 0, then the mask or-ed over everything"""
    x = np.full(n, fill, np.uint8) if width == 0 else base[width][:n].copy()
    assert x.size == n
    x = plant(x, preamble, at)
    if flip_at >= 0:
        x[flip_at] ^= flip_xor
    return x | np.uint8(mask)


def golden_cases(path):
    """tests/golden/preamble.npz (make_preamble_golden.py) unpacked: (tile, halo, [case]) with a case a dict of name, preamble, x, at,
    cuts (None for one work() on the whole stream per threshold) and calls: [(threshold, elements handed, consumed, reserve, forwarded,
    label indices as uint64)]"""
    g = np.load(path)
    base = {1: g["base1"], 8: g["base8"]}
    starts = np.concatenate([[0], np.cumsum(g["calls"][:, 6])])
    assert starts[-1] == g["label_delta"].size
    out = []
    for name, row in zip(g["names"].tolist(), g["spec"].tolist()):
        width, n, fill, mask, flip_at, flip_xor, pre_off, P, at_off, n_at, call_off, n_calls, is_cuts = row
        pre = g["pre_all"][pre_off:pre_off + P]
        at = g["at_all"][at_off:at_off + n_at].tolist()
        calls = []
        for k in range(call_off, call_off + n_calls):
            thr, handed, consumed, reserve, forwarded, off, count = g["calls"][k].tolist()
            assert off == starts[k]
            calls.append((thr, handed, consumed, reserve, forwarded, np.cumsum(g["label_delta"][off:off + count], dtype=np.uint64)))
        out.append(dict(name=name, preamble=pre, x=golden_stream(base, width, n, fill, mask, flip_at, flip_xor, pre, at), at=at,
                        cuts=[c[1] - (p[1] - p[2]) for p, c in zip([(0, 0, 0)] + calls, calls)] if is_cuts else None, calls=calls))
    return int(g["tile"]), int(g["halo"]), out


def run_cuts(work, stream, cuts, P):
    """The scheduler's side of a stream cut into work() calls: every call sees what the block left unconsumed followed by the next
    cut.  work(buffer) -> (consumed, label indices relative to the buffer).  Returns (labels shifted by what was consumed before
    their call, total consumed)."""
    held = np.zeros(0, np.uint8)
    labels, done, at = [], 0, 0
    for c in cuts:
        held = np.concatenate([held, stream[at:at + c]])
        at += c
        consumed, idx = work(held)
        assert consumed == positions(held.size, P)
        labels.extend(int(i) + done for i in idx)
        done += consumed
        held = held[consumed:]
    return np.array(labels, np.uint64), done
