"""Model of /comms/scrambler and /comms/descrambler: digital/lfsr.h, Scrambler.cpp and Descrambler.cpp restated on Python integers.

  Lfsr / glfsr_init / Model   the reference's register and block loops, one bit per step: lfsr_t's three long long words kept as
                              unsigned 64-bit values, the mask found by an ARITHMETIC right shift of 1 << 63 (every bit from the
                              polynomial's top bit upward) and kept when the polynomial has no bit in 63..1
  plan                        SCAN when the polynomial owns the mask's lowest bit m and 0 <= seed < 2^m, SERIAL otherwise
  jump                        the additive register n steps ahead by matrix powers over GF(2)
  window_check                long streams: for every i >= m the state in front of bit i rebuilt from the m (ret, u) pairs before it,
                              its bit m-1 compared with in[i] ^ out[i]; numpy arrays or torch tensors on the device
  state_from_tail             the register behind a stream from its last m pairs

Under SCAN the state stays below 2^m, ret is bit m-1 of the old state, and D' = ((D << 1) mod 2^m) ^ ret * P' ^ u with P' the
polynomial without bit m and u = 0 (additive), in (multiplicative scrambler: bit 0 becomes out) or out (multiplicative descrambler:
bit 0 becomes in).  Whatever lay in the register m steps back has been shifted out, which is what the window check rests on.
"""
import numpy as np

U64 = (1 << 64) - 1
KINDS = ("additive", "scrambler", "descrambler")      # the three recurrences


def u64(v):
    return int(v) & U64


class Lfsr:
    def __init__(self):
        self.data = self.polynomial = self.mask = 0       # the constructor's memset


def glfsr_init(l, polynom, seed):
    """lfsr.h:63-83"""
    polynom = u64(polynom)
    l.polynomial = polynom | 1
    l.data = u64(seed)
    seed_mask = 1 << 63
    for _ in range(63):                                   # while (shift--), shift = 63
        if polynom & seed_mask:
            l.mask = seed_mask
            break
        seed_mask = (seed_mask >> 1) | (1 << 63)          # signed: the sign bit is shifted in
    return l


def lowest_bit(mask):
    return (mask & -mask).bit_length() - 1


def plan(l):
    """the plan rule on a register as glfsr_init left it (data = the seed)"""
    if l.mask == 0:
        return "SERIAL"
    m = lowest_bit(l.mask)
    return "SCAN" if (l.polynomial >> m) == 1 and (l.data >> m) == 0 else "SERIAL"


def kind_of(descramble, mode):
    return "additive" if mode == "additive" else ("descrambler" if descramble else "scrambler")


class Model:
    """the block: constructor defaults, setPoly / setSeed (each GLFSR_init with both values), setMode, work()"""

    def __init__(self, descramble=False, mode="multiplicative", poly=0x19, seed=1):
        self.descramble = bool(descramble)
        self.l = Lfsr()
        self._polynom, self._seed = 1, 1
        self.set_mode("multiplicative")
        self.set_poly(0x19)
        self.set_mode(mode)
        if seed != 1:
            self.set_seed(seed)
        if poly != 0x19:
            self.set_poly(poly)

    def set_poly(self, poly):
        self._polynom = poly
        glfsr_init(self.l, self._polynom, self._seed)

    def set_seed(self, seed):
        self._seed = seed
        glfsr_init(self.l, self._polynom, self._seed)

    def set_mode(self, mode):
        if mode not in ("additive", "multiplicative"):
            raise ValueError("unknown mode: %s" % mode)
        self.mode = mode

    def plan(self):
        """of the register as it stands: meaningful right after set_poly / set_seed"""
        return plan(self.l)

    def process(self, x):
        """work()'s loop over the bytes of x (only bit 0 counts); returns the output bytes"""
        kind = kind_of(self.descramble, self.mode)
        data, mask, pol = self.l.data, self.l.mask, self.l.polynomial
        bits = (np.asarray(x, dtype=np.uint8) & 1).tolist()
        out = [0] * len(bits)
        for i, b in enumerate(bits):
            data = (data << 1) & U64
            ret = 0
            if data & mask:
                ret = 1
                data ^= pol
            o = b ^ ret
            if kind == "scrambler":
                data = (data & ~1) | o
            elif kind == "descrambler":
                data = (data & ~1) | b
            out[i] = o
        self.l.data = data
        return np.array(out, dtype=np.uint8)


# ---- matrix powers over GF(2) (additive register under SCAN): a matrix is its 64 columns
def step_columns(polynomial, m):
    return [(((1 << c) << 1) ^ (polynomial if c == m - 1 else 0)) & U64 if c < m else 0 for c in range(64)]


def mat_vec(cols, v):
    acc, c = 0, 0
    while v:
        if v & 1:
            acc ^= cols[c]
        v >>= 1
        c += 1
    return acc


def mat_mul(a, b):
    return [mat_vec(a, col) for col in b]


def jump(state, n, polynomial, m):
    """the additive register n steps on from `state` (< 2^m)"""
    sq = step_columns(polynomial, m)
    while n:
        if n & 1:
            state = mat_vec(sq, state)
        n >>= 1
        if n:
            sq = mat_mul(sq, sq)
    return state


# ---- long streams
def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _pairs(inp, out, kind):
    ret = (inp & 1) ^ out
    u = None if kind == "additive" else ((inp & 1) if kind == "scrambler" else out)
    return ret, u


def _rebuild(ret, u, n_out, polynomial, m):
    """D_i mod 2^64 for i = m ... m + n_out - 1 of a piece, from the m pairs in front of each"""
    pp = (polynomial & ~(1 << m)) & U64
    if _is_torch(ret):
        import torch
        pp = pp - (1 << 64) if pp >= (1 << 63) else pp
        D = torch.zeros(n_out, dtype=torch.int64, device=ret.device)
        for j in range(m):
            r = ret[j:j + n_out].to(torch.int64)
            D = (D << 1) ^ ((-r) & pp)
            if u is not None:
                D = D ^ u[j:j + n_out].to(torch.int64)
        return D
    D = np.zeros(n_out, dtype=np.uint64)
    for j in range(m):
        r = ret[j:j + n_out].astype(np.uint64)
        D = (D << np.uint64(1)) ^ ((np.uint64(0) - r) & np.uint64(pp))
        if u is not None:
            D = D ^ u[j:j + n_out].astype(np.uint64)
    return D


def window_check(inp, out, polynomial, m, kind, piece=1 << 24):
    """the number of i >= m whose in[i] ^ out[i] is not bit m-1 of the state rebuilt from the m pairs before i (0: none)"""
    n = int(inp.shape[0])
    bad = 0
    for a in range(m, n, piece):
        b = min(n, a + piece)
        ret, u = _pairs(inp[a - m:b], out[a - m:b], kind)
        D = _rebuild(ret, u, b - a, polynomial, m)
        if _is_torch(ret):
            import torch
            pred = ((D >> (m - 1)) & 1).to(torch.uint8)
            bad += int((pred != ret[m:]).sum().item())
        else:
            pred = ((D >> np.uint64(m - 1)) & np.uint64(1)).astype(np.uint8)
            bad += int(np.count_nonzero(pred != ret[m:]))
    return bad


def state_from_tail(inp, out, polynomial, m, kind):
    """the register behind the stream (SCAN, at least m bits long) from its last m pairs"""
    n = int(inp.shape[0])
    assert n >= m
    ret, u = _pairs(inp[n - m:], out[n - m:], kind)
    D = _rebuild(ret, u, 1, polynomial, m)
    return int(D[0].item()) & ((1 << m) - 1)


# ---- the fixture (tests/golden/scrambler.npz, written by tests/golden/make_scrambler_golden.py)
def case_ops(cfg, cuts):
    """the calls of a fixture case, cfg = [descramble, mode, has_pre, pre_poly, poly, seed, serial]: the configuration (setMode; setPoly(pre)
    where the case is about a retained mask; setSeed; setPoly), then work() over the cuts with setSeed after the third and setPoly
    after the fourth, both with the case's own values -- the register starts over in mid-stream"""
    _, mode, has_pre, pre, poly, seed, _ = [int(v) for v in cfg]
    ops = [("mode", "multiplicative" if mode else "additive")]
    if has_pre:
        ops.append(("poly", pre))
    ops += [("seed", seed), ("poly", poly)]
    for k, c in enumerate(int(c) for c in cuts):
        ops.append(("work", c))
        if k == 2:
            ops.append(("seed", seed))
        if k == 3:
            ops.append(("poly", poly))
    return ops


def run_case(cfg, cuts, x):
    """the model over a fixture case: (outputs, final data, mask, plan right after the configuration)"""
    m = Model(descramble=bool(int(cfg[0])))
    outs, pos, plan_at_start = [], 0, None
    for op, v in case_ops(cfg, cuts):
        if op == "work":
            if plan_at_start is None:
                plan_at_start = m.plan()
            outs.append(m.process(x[pos:pos + v]))
            pos += v
        else:
            getattr(m, "set_" + op)(v)
    return np.concatenate(outs), m.l.data, m.l.mask, plan_at_start
