"""numpy model of /comms/bits_to_symbols, /comms/symbols_to_bits, /comms/bytes_to_symbols and /comms/symbols_to_bytes in this
project's own formulation: bit matrices for the three clean conversions, the clipped OR for symbols -> bytes.  Also the
group table (what the reference reserves) and the label ratios.  tests/golden/repack.npz holds what the reference's loops give."""
import numpy as np

KINDS = ("bits_to_symbols", "symbols_to_bits", "bytes_to_symbols", "symbols_to_bytes")
ORDERS = ("MSBit", "LSBit")
WIDTHS = tuple(range(1, 9))
# the constructors' values: modulus 1 and this order
FRESH_ORDER = {"bits_to_symbols": "MSBit", "symbols_to_bits": "MSBit", "bytes_to_symbols": "LSBit", "symbols_to_bytes": "LSBit"}
RESERVE_BYTES = {1: 1, 2: 1, 3: 3, 4: 1, 5: 5, 6: 3, 7: 7, 8: 1}      # bytes -> symbols
RESERVE_SYMS = {1: 8, 2: 4, 3: 8, 4: 2, 5: 8, 6: 4, 7: 8, 8: 1}       # symbols -> bytes


def group(kind, w):
    """(in, out): the indivisible unit in input and output elements"""
    if kind == "bits_to_symbols":
        return w, 1
    if kind == "symbols_to_bits":
        return 1, w
    if kind == "bytes_to_symbols":
        return RESERVE_BYTES[w], RESERVE_BYTES[w] * 8 // w
    return RESERVE_SYMS[w], RESERVE_SYMS[w] * w // 8


def reserve(kind, w):
    """what work() sets on the input port (None: nothing)"""
    return None if kind == "symbols_to_bits" else group(kind, w)[0]


def label_ratio(kind, w):
    """(mult, div) of label.toAdjusted"""
    return {"bits_to_symbols": (1, w), "symbols_to_bits": (w, 1), "bytes_to_symbols": (8, w), "symbols_to_bytes": (w, 8)}[kind]


def out_elems(kind, w, n):
    gin, gout = group(kind, w)
    assert n % gin == 0, "not a whole group"
    return n // gin * gout


def work_sizes(kind, w, in_elems, out_elems_):
    """(consumed, produced) of one work() call"""
    gin, gout = group(kind, w)
    g = min(in_elems // gin, out_elems_ // gout)
    return g * gin, g * gout


def _shifts(n, order):
    """the bit of an n-bit value that the k-th bit of the stream sits on"""
    return np.arange(n - 1, -1, -1) if order == "MSBit" else np.arange(n)


def _symbols_of_bits(bits, w, order):
    return (bits.reshape(-1, w).astype(np.uint32) << _shifts(w, order)).sum(axis=1).astype(np.uint8)


def _bits_of_values(x, n, order):
    return ((x.astype(np.uint32)[:, None] >> _shifts(n, order)) & 1).astype(np.uint8).reshape(-1)


def bits_to_symbols(x, w, order):
    return _symbols_of_bits((np.asarray(x, np.uint8) != 0).astype(np.uint8), w, order)


def symbols_to_bits(x, w, order):
    return _bits_of_values(np.asarray(x, np.uint8), w, order)


def bytes_to_symbols(x, w, order):
    return _symbols_of_bits(_bits_of_values(np.asarray(x, np.uint8), 8, order), w, order)


def symbols_to_bytes(x, w, order):
    """THE CLIPPED OR.  Eight symbols and their w bytes are one number G of 8 w bits (little-endian bytes in LSBit order, big-endian in
    MSBit order) in which field k = bits [w k, w k + w) belongs to symbol k (LSBit) or 7 - k (MSBit).  The whole 8-bit value of that
    symbol is placed with its bit 0 on bit w k and cut off at the upper edge of the last byte the field touches."""
    s = np.asarray(x, np.uint8).reshape(-1, 8).astype(np.uint64)
    G = np.zeros(s.shape[0], np.uint64)
    for k in range(8):
        p = w * k
        end = min(p + 8, 8 * ((p + w - 1) // 8 + 1))
        mask = np.uint64(((1 << end) - 1) ^ ((1 << p) - 1))
        G |= (s[:, 7 - k if order == "MSBit" else k] << np.uint64(p)) & mask
    byte_shifts = (8 * _shifts(w, order)).astype(np.uint64)
    return ((G[:, None] >> byte_shifts) & np.uint64(255)).astype(np.uint8).reshape(-1)


FUNCS = {"bits_to_symbols": bits_to_symbols, "symbols_to_bits": symbols_to_bits, "bytes_to_symbols": bytes_to_symbols,
         "symbols_to_bytes": symbols_to_bytes}


def convert(kind, x, w, order):
    x = np.asarray(x, np.uint8)
    out_elems(kind, w, x.size)
    if kind == "symbols_to_bytes" and x.size % 8:
        # (groups of 1, 2 or 4 symbols: pad to the model's eight; a value never reaches beyond the byte its field ends in)
        pad = (-x.size) % 8
        return symbols_to_bytes(np.concatenate([x, np.zeros(pad, np.uint8)]), w, order)[:x.size * w // 8]
    return FUNCS[kind](x, w, order)


def case_name(kind, order, w):
    return "%s/%s/%d" % (kind, order, w)


CASES = [case_name(k, o, w) for k in KINDS for o in ORDERS for w in WIDTHS]
