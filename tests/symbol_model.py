"""numpy restatements of the four loops behind /comms/symbol_mapper, /comms/symbol_slicer, /comms/differential_encoder and
/comms/differential_decoder (reference digital/SymbolMapper.cpp:89-91, SymbolSlicer.cpp:43-52 and :88-97, DifferentialEncoder.cpp:59-63,
DifferentialDecoder.cpp:59-64).  Test infrastructure: the product never imports it.

Streams: a real stream of scalar type T is an (n,) array of T, a complex one an (n, 2) array of T (re, im).  Maps have the same layout.

The slicer's distance is written with explicit float32 steps: the difference in the promoted element type (int64 here for every
integer type, which holds every difference that does not overflow the reference's own int / long), its conversion to float32 (round to
nearest even), and for complex types two float32 products and one float32 sum, each rounded on its own.

The encoder comes twice: the step as the reference writes it (encoder_steps) and the modular prefix sum (encoder_scan) that holds
whenever encoder_plan(symbols) says SCAN -- the check of all 65536 (in, last) pairs that the handle runs as well."""
import numpy as np

SCAN, SERIAL = 0, 1
TYPES = [(s, c) for s in ("float64", "float32", "int64", "int32", "int16", "int8") for c in (False, True)]
FLT_MAX = np.float32(3.4028234663852886e38)
U32 = (1 << 32) - 1


def type_name(scalar, cplx):
    return ("complex_" if cplx else "") + scalar


# ---- mapper
def mapper_mask(n):
    """(unsigned char)((1 << log2(n)) - 1), SymbolMapper.cpp:76"""
    if n == 0:
        raise ValueError("Map must be nonzero size")
    if n & (n - 1):
        raise ValueError("Map must be a power of two in length")
    return (n - 1) & 255


def mapper(m, x):
    m = np.asarray(m)
    return m[np.asarray(x, dtype=np.uint8) & np.uint8(mapper_mask(m.shape[0]))]


# ---- slicer
def _promote(a):
    return a.astype(np.int64) if a.dtype.kind == "i" else a


def _to_f32(d):
    with np.errstate(over="ignore", invalid="ignore"):
        return d.astype(np.float32)


def distance(mj, x):
    """float32 distances of every sample of x to the one map entry mj"""
    x = _promote(np.asarray(x))
    mj = _promote(np.asarray(mj))
    with np.errstate(over="ignore", invalid="ignore"):
        if x.ndim == 1:
            return _to_f32(np.abs(mj - x))
        dr = _to_f32(mj[0] - x[:, 0])
        di = _to_f32(mj[1] - x[:, 1])
        a = dr * dr
        b = di * di
        assert a.dtype == np.float32 and b.dtype == np.float32
        return a + b


def slicer(m, x):
    m, x = np.asarray(m), np.asarray(x)
    if m.shape[0] == 0:
        raise ValueError("Map must be nonzero size")
    best = np.full(x.shape[0], FLT_MAX, dtype=np.float32)
    idx = np.zeros(x.shape[0], dtype=np.int64)
    for j in range(m.shape[0]):
        d = distance(m[j], x)
        with np.errstate(invalid="ignore"):
            win = d < best
        best = np.where(win, d, best)
        idx = np.where(win, j, idx)
    return (idx & 255).astype(np.uint8)


# ---- differential coders
def encoder_step(b, last, symbols):
    return (((int(b) + int(last) + int(symbols)) & U32) % int(symbols)) & 255


def encoder_steps(x, symbols, last=0):
    """the reference's loop; returns (out, carried byte)"""
    out = np.zeros(len(x), dtype=np.uint8)
    for i, b in enumerate(x):
        last = encoder_step(b, last, symbols)
        out[i] = last
    return out, last


def encoder_plan(symbols):
    """SCAN when the step equals (in + last) mod min(symbols, 256) for all 65536 pairs of bytes"""
    symbols = int(symbols)
    m = min(symbols, 256)
    s = np.arange(256, dtype=np.int64)[:, None] + np.arange(256, dtype=np.int64)[None, :]
    step = (((s + symbols) & U32) % symbols) & 255
    return SCAN if np.array_equal(step, s % m) else SERIAL


def encoder_scan(x, symbols, last=0):
    """the prefix-sum form (only where encoder_plan says SCAN); returns (out, carried byte)"""
    m = min(int(symbols), 256)
    x = np.asarray(x, dtype=np.uint8)
    if x.size == 0:
        return np.zeros(0, np.uint8), last
    out = ((np.cumsum(x, dtype=np.uint64) + np.uint64(last)) % np.uint64(m)).astype(np.uint8)
    return out, int(out[-1])


def encoder(x, symbols, last=0):
    return encoder_scan(x, symbols, last) if encoder_plan(symbols) == SCAN else encoder_steps(x, symbols, last)


def decoder(x, symbols, last=0):
    """returns (out, carried byte)"""
    x = np.asarray(x, dtype=np.uint8)
    if x.size == 0:
        return np.zeros(0, np.uint8), last
    cur = x.astype(np.int64)
    prev = np.concatenate([[int(last)], cur[:-1]])
    out = ((((cur - prev + int(symbols)) & U32) % int(symbols)) & 255).astype(np.uint8)
    return out, int(x[-1])


# ---- the fixture's coder scenario (tests/golden/make_symbols_golden.py)
CODER_SYMBOLS = [1, 2, 3, 4, 7, 256, 257, 300, 510, 511, 65536, 2 ** 32 - 511, 2 ** 32 - 510, 2 ** 32 - 256, 2 ** 32 - 1]
CODER_CUTS = [1, 37, 100, 11, 851]


def coder_ops(symbols):
    """two calls at 256 symbols, so that the carried byte is any byte, then setSymbols(symbols) and three more calls"""
    c = CODER_CUTS
    return [("s", 256), ("w", c[0]), ("w", c[1]), ("s", int(symbols)), ("w", c[2]), ("w", c[3]), ("w", c[4])]


def run_coder(decode, ops, x, step_form=False):
    """(out, carried byte) of a sequence of setSymbols / work calls from a fresh block"""
    symbols, last, pos, outs = 2, 0, 0, []
    for op, v in ops:
        if op == "s":
            symbols = v
            continue
        piece = x[pos:pos + v]
        if decode:
            o, last = decoder(piece, symbols, last)
        elif step_form:
            o, last = encoder_steps(piece, symbols, last)
        else:
            o, last = encoder(piece, symbols, last)
        outs.append(o)
        pos += v
    return np.concatenate(outs), last
