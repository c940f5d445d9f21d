"""Model of /comms/preamble_framer and /comms/frame_insert: the yardstick of tests/test_framer_cpu.py and
tests/test_framer_gpu.py.  Integer and byte work only, so every comparison against it is exact.  Two formulations:

  walk   the loop over the labels, as the blocks' work() is written: a list of chunks (runs of the input, inserts), concatenated
  map    independently: the input position and the length of every insert by prefix sums, then the source of EVERY output index by
         searchsorted over the positions at which the inserts begin

A stream is an array of rows, one element per row, es bytes each (rows(x)); an event is (index, width, kind, length) with kind in
"other", "start", "end"; a configuration is Config(preamble rows, symbol width, header?, header id, padding).  Both formulations follow
the same rules: an event at or behind the end of the input is left alone; the shift of the labels grows by a start event's insert at
the next event with a different index; an end event's head runs to index + width, clipped; a head never runs backwards; events are
taken in groups that fit the capacity whole, with the element their last label sits on (include/pcx.h, pcx_framer_plan).

The header coder comes with its decoder (single-bit correction per Hamming word), which a frame synchroniser will need too.

tests/golden/framer.npz (tests/golden/make_framer_golden.py; `golden_cases` unpacks it) holds what the reference's own blocks posted.
Both formulations equal it wherever no head would run backwards.  Its header part pins `header_bits` to the reference's
encodeHeaderWord and `header_decode` to its decodeHeaderWord on 756 words with no, one and two flipped bits: the pin a frame
synchroniser's decoder can rely on."""
import collections

import numpy as np

HEADER_BITS = 58
Config = collections.namedtuple("Config", "preamble width header header_id padding")
Result = collections.namedtuple("Result", "consumed out_len used insert_at shift cut error")


# ---- the header
def checksum8(values):
    acc = 0
    for v in values:
        acc = ((acc >> 1) | ((acc & 1) << 7)) & 0xFF
        acc = (acc + v) & 0xFF
    return acc


def header_checksum(header_id, length):
    return checksum8([header_id & 0xFF, length & 0xFF, (length >> 8) & 0xFF])


# code bit k of a Hamming(8,4) word as the parity of the data bits in PARITY[k]
PARITY = [(0, 1, 3), (0, 2, 3), (0,), (1, 2, 3), (1,), (2,), (3,), (0, 1, 2)]
DATA_AT = (2, 4, 5, 6)          # where the four data bits sit


def hamming_encode(nibble):
    return [sum((nibble >> d) & 1 for d in taps) & 1 for taps in PARITY]


def hamming_decode(b):
    """eight code bits -> (nibble, uncorrectable?)"""
    b = list(b)
    s = ((b[0] + b[2] + b[4] + b[6]) & 1) | ((b[1] + b[2] + b[5] + b[6]) & 1) << 1 | ((b[3] + b[4] + b[5] + b[6]) & 1) << 2
    overall = sum(b) & 1
    bad = False
    if overall:                 # one bit flipped: the syndrome names it (0: the overall parity bit itself)
        b[7 if s == 0 else s - 1] ^= 1
    elif s:
        bad = True              # two bits flipped
    return sum(b[p] << k for k, p in enumerate(DATA_AT)), bad


def header_bits(header_id, length):
    """the 58 bits: 0, 1, then id, TWELVE bits of the length, and the checksum over the id and all SIXTEEN bits of the length"""
    chk = header_checksum(header_id, length)
    nibbles = [header_id & 15, (header_id >> 4) & 15, length & 15, (length >> 4) & 15, (length >> 8) & 15, chk & 15, (chk >> 4) & 15]
    bits = [0, 1]
    for nb in nibbles:
        bits += hamming_encode(nb)
    assert len(bits) == HEADER_BITS
    return bits


def header_word(header_id, length):
    return sum(b << i for i, b in enumerate(header_bits(header_id, length)))


def header_decode(bits):
    """58 bits -> (id, the twelve length bits, checksum, uncorrectable?)"""
    nib, bad = [], False
    for k in range(7):
        v, e = hamming_decode(bits[2 + 8 * k:10 + 8 * k])
        nib.append(v)
        bad |= e
    return nib[0] | nib[1] << 4, nib[2] | nib[3] << 4 | nib[4] << 8, nib[5] | nib[6] << 4, bad


# ---- streams as rows of bytes
def rows(x):
    """(n,) uint8 -> (n, 1); (n, 2) float32 / float64 or (n,) complex -> (n, 8) / (n, 16) uint8"""
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint8 and x.ndim == 1:
        return x.reshape(-1, 1)
    if np.iscomplexobj(x):
        x = x.view(x.real.dtype).reshape(-1, 2)
    assert x.ndim == 2 and x.shape[1] == 2 and x.dtype in (np.float32, np.float64)
    return x.view(np.uint8).reshape(x.shape[0], 2 * x.dtype.itemsize)


def unrows(r, like):
    """rows back to the layout of `like`: (n,) uint8 or (n, 2) of its float type"""
    if r.shape[1] == 1:
        return r.reshape(-1)
    return np.ascontiguousarray(r).view(np.float32 if r.shape[1] == 8 else np.float64).reshape(-1, 2)


def negated(row):
    """a complex element with the sign bit of both components flipped"""
    out = row.copy()
    half = row.shape[0] // 2
    out[half - 1] ^= 0x80
    out[2 * half - 1] ^= 0x80
    return out


def insert_rows(cfg, length):
    """what a start event inserts: every preamble symbol `width` times, then the header symbols"""
    pre = np.repeat(cfg.preamble, cfg.width, axis=0)
    if not cfg.header:
        return pre
    sym = cfg.preamble[-1]
    hdr = np.stack([sym if b else negated(sym) for b in header_bits(cfg.header_id, length & 0xFFFF)])
    return np.concatenate([pre, hdr])


def insert_len(cfg):
    return cfg.preamble.shape[0] * cfg.width + (HEADER_BITS if cfg.header else 0)


# ---- formulation 1: the walk
def walk(x, events, cfg, cap=None):
    """-> (output rows, Result)"""
    n, P, pad = x.shape[0], insert_len(cfg), cfg.padding
    cap = n + len(events) * (P + pad) if cap is None else cap
    ne = len(events)
    used, at, shift_of = [False] * ne, [0] * ne, [0] * ne
    st = dict(consumed=0, out=0, shift=0, need=0, found=None, chunks=[])

    def handle(s, i):
        index, width, kind, length = events[i]
        if s["found"] is not None and s["found"] != index:
            s["found"] = None
            s["shift"] += P
        if kind == "start":
            head = max(index - s["consumed"], 0)
            s["chunks"] = s["chunks"] + [x[s["consumed"]:s["consumed"] + head]]
            at[i] = s["out"] + head
            s["chunks"] = s["chunks"] + [insert_rows(cfg, length)]
            s["consumed"] += head
            s["out"] += head + P
            s["found"] = index
        elif kind == "end":
            head = max(min(index + width, n) - s["consumed"], 0)
            s["chunks"] = s["chunks"] + [x[s["consumed"]:s["consumed"] + head], np.zeros((pad, x.shape[1]), np.uint8)]
            at[i] = s["out"] + head
            s["consumed"] += head
            s["out"] += head + pad
            s["shift"] += pad
        else:
            at[i] = index + s["shift"]
        shift_of[i] = s["shift"]
        s["need"] = max(s["need"], index + 1)

    cut, error, i = False, None, 0
    tail = None
    while i < ne:
        if events[i][0] >= n:
            i += 1
            continue
        t, j = dict(st), i
        while True:
            handle(t, j)
            j += 1
            if not (j < ne and events[j][0] < max(t["consumed"], t["need"])):
                break
        through = max(t["need"] - t["consumed"], 0)
        if t["out"] + through <= cap:
            for k in range(i, j):
                used[k] = True
            st, i = t, j
            continue
        stop = max(events[i][0], st["consumed"])
        alone = t["out"] - st["out"] + through - (stop - st["consumed"])
        if alone > cap:
            error = "the inserts at index %d need %d output elements, the output buffer holds %d" % (events[i][0], alone, cap)
            return None, Result(0, 0, [False] * ne, [0] * ne, [0] * ne, False, error)
        cut, tail = True, min(stop - st["consumed"], cap - st["out"])
        break
    if tail is None:
        tail = min(n - st["consumed"], cap - st["out"])
    chunks = st["chunks"] + [x[st["consumed"]:st["consumed"] + tail]]
    out = np.concatenate(chunks) if chunks else x[:0]
    for k in range(ne):
        if not used[k]:
            at[k] = shift_of[k] = 0
    return out, Result(st["consumed"] + tail, st["out"] + tail, used, at, shift_of, cut, None)


# ---- formulation 2: the map
def index_map(x, events, cfg, cap=None):
    """-> (output rows, Result), by arrays: no loop over the events besides the one that finds the groups"""
    n, P, pad = x.shape[0], insert_len(cfg), cfg.padding
    ne = len(events)
    cap = n + ne * (P + pad) if cap is None else cap
    idx = np.array([e[0] for e in events], np.int64).reshape(-1)
    wid = np.array([e[1] for e in events], np.int64).reshape(-1)
    is_start = np.array([e[2] == "start" for e in events], bool).reshape(-1)
    is_end = np.array([e[2] == "end" for e in events], bool).reshape(-1)
    live = np.flatnonzero(idx < n)                  # the events of this call, by their place in the list
    li, ls, le = idx[live], is_start[live], is_end[live]
    m = live.size
    # where the input stands when an event's insert is made: a running maximum, since a head never runs backwards
    reach = np.where(ls, li, np.where(le, np.minimum(li + wid[live], n), 0))
    pos = np.maximum.accumulate(reach) if m else reach
    length = np.where(ls, P, np.where(le, pad, 0))
    before = np.cumsum(length) - length             # inserted elements in front of an event's insert
    begin = pos + before                            # where the insert begins in the output
    out_after = begin + length
    need = np.maximum.accumulate(li + 1) if m else li
    through = np.maximum(need - pos, 0)
    # the shift: the paddings up to and including the event, and one insert length for every run of start events that an event with
    # another index has followed
    bump = np.zeros(m, np.int64)
    for k in np.flatnonzero(ls):
        later = np.flatnonzero(li[k + 1:] != li[k])
        if later.size:
            bump[k + 1 + later[0]] = 1
    shift = P * np.cumsum(bump) + pad * np.cumsum(le)
    # groups: an event opens one when it lies at or behind everything passed on and every index handled so far
    opens = np.ones(m, bool)
    if m > 1:
        opens[1:] = li[1:] >= np.maximum(pos[:-1], need[:-1])
    first = np.flatnonzero(opens)                   # the first event of every group
    last = np.append(first[1:], m) - 1              # and its last
    fits = out_after[last] + through[last] <= cap if m else np.zeros(0, bool)
    ngroups = int(np.argmin(fits)) if (m and not fits.all()) else first.size
    cut = ngroups < first.size
    kept = int(first[ngroups]) if cut else m        # events handled
    consumed0 = int(pos[kept - 1]) if kept else 0
    out0 = int(out_after[kept - 1]) if kept else 0
    if cut:
        g0, g1 = int(first[ngroups]), int(last[ngroups])
        stop = max(int(li[g0]), consumed0)
        alone = int(out_after[g1]) - out0 + int(through[g1]) - (stop - consumed0)
        if alone > cap:
            error = "the inserts at index %d need %d output elements, the output buffer holds %d" % (li[g0], alone, cap)
            return None, Result(0, 0, [False] * ne, [0] * ne, [0] * ne, False, error)
        tail = min(stop - consumed0, cap - out0)
    else:
        tail = min(n - consumed0, cap - out0)
    consumed, out_len = consumed0 + tail, out0 + tail
    # every output index to its source
    b, ln, bf = begin[:kept], length[:kept], before[:kept]
    t = np.arange(out_len, dtype=np.int64)
    k = np.searchsorted(b, t, side="right") - 1     # the last insert that begins at or in front of t
    inside = (k >= 0) & (t < (b[k] + ln[k] if kept else 0))
    src = t - np.where(k >= 0, (bf + ln)[k] if kept else 0, 0)      # the input element, where t is not inside an insert
    out = np.zeros((out_len, x.shape[1]), np.uint8)
    out[~inside] = x[src[~inside]]
    for e in np.flatnonzero(ls[:kept]):             # the inserted rows themselves (padding stays zero)
        sel = inside & (k == e)
        out[sel] = insert_rows(cfg, events[live[e]][3])[(t - b[e])[sel]]
    used, at, sh = [False] * ne, [0] * ne, [0] * ne
    for e in range(kept):
        used[live[e]] = True
        at[live[e]] = int(begin[e]) if (ls[e] or le[e]) else int(li[e] + shift[e])
        sh[live[e]] = int(shift[e])
    return out, Result(consumed, out_len, used, at, sh, cut, None)


def expected_labels(events, res):
    """(event position, output index) of the labels the block posts"""
    return [(i, events[i][0] + res.shift[i]) for i in range(len(events)) if res.used[i]]


# ---- the recorded reference (tests/golden/framer.npz, written by tests/golden/make_framer_golden.py)
GOLDEN_TYPES = ("uint8", "complex_float32", "complex_float64")
DATA_KINDS = (None, "integer", "string")        # what a label carries: nothing, an unsigned integer, a string


def golden_input(dtype, n):
    """the rows of the n input elements of a recorded case: every element carries its own position.  Bytes are 2 + i % 251, complex
    elements (i, -(i + 0.5))"""
    i = np.arange(n)
    if dtype == "uint8":
        return rows((2 + i % 251).astype(np.uint8))
    return rows(np.stack([i, -(i + 0.5)], axis=1).astype(np.float32 if dtype == "complex_float32" else np.float64))


def golden_output(x, src_delta, literals):
    """the recorded output rows from their compact form: src (the running sum of src_delta) names the input row an output row equals,
    -1 stands for the next of the literal rows"""
    src = np.cumsum(src_delta, dtype=np.int64)
    out = np.zeros((src.size, x.shape[1]), np.uint8)
    out[src >= 0] = x[src[src >= 0]]
    out[src < 0] = literals
    return out


def label_events(labels, start_id, end_id):
    """[(id, index, width, data)] -> events, by the blocks' rules: the start id is tested before the end id; the header's length is
    data * width cut to sixteen bits where the data is an integer, else 0"""
    return [(index, width, "start" if i == start_id else "end" if i == end_id else "other", (data * width) & 0xFFFF if isinstance(data, int) else 0)
            for i, index, width, data in labels]


def golden_cases(path):
    """-> (tile bytes, [case], header): a case is a dict of name, dtype, n, x (rows), preamble (as the element type: (P,) uint8 or (P, 2)),
    cfg (a Config), start_id, end_id, labels [(id, index, width, data)], events, backward, leaves (the reference posted a chunk that
    leaves its input: nothing else is recorded), consumed, out (rows) and posted [(place of the input label, index, width, kind of data)].
    header holds the header coder's and decoder's recordings (see the maker).  These are the pin a frame synchroniser's decoder can rely
    on: dec rows are (word, id, twelve length bits, checksum, error flag) of the reference's decodeHeaderWord."""
    g = np.load(path)
    lit = {t: g["lit_" + t] for t in GOLDEN_TYPES}
    out = []
    for k, (name, row) in enumerate(zip(g["names"].tolist(), g["case"].tolist())):
        (tcode, n, width, hid, padding, P, pre_off, lab_off, n_lab, leaves, backward, consumed, out_rows, src_off, lit_off, n_lit, post_off, n_post) = row
        t = GOLDEN_TYPES[tcode]
        if t == "uint8":
            pre = g["pre_u8"][pre_off:pre_off + P]
        else:
            pre = g["pre_c"][pre_off:pre_off + P].astype(np.float32 if t == "complex_float32" else np.float64)
        labels = []
        for j in range(lab_off, lab_off + n_lab):
            index, w, kind, value = g["label_num"][j].tolist()
            labels.append((str(g["label_id"][j]), index, w, None if kind == 0 else value if kind == 1 else str(g["label_text"][j])))
        sid, eid = str(g["start_id"][k]), str(g["end_id"][k])
        x = golden_input(t, n)
        out.append(dict(name=name, dtype=t, n=n, x=x, preamble=pre, cfg=Config(rows(pre), width, t != "uint8", hid, padding), start_id=sid, end_id=eid,
                        labels=labels, events=label_events(labels, sid, eid), backward=bool(backward), leaves=bool(leaves), consumed=consumed,
                        out=golden_output(x, g["src"][src_off:src_off + out_rows], lit[t][lit_off:lit_off + n_lit]),
                        posted=[tuple(p) for p in g["posted"][post_off:post_off + n_post].tolist()]))
    header = dict(enc=[(i, ln, int(w)) for (i, ln), w in zip(g["enc_in"].tolist(), g["enc_word"].tolist())],
                  enc_all=dict(zip(g["enc_all_id"].tolist(), g["enc_all_sha"].tolist())), dec=[tuple(int(v) for v in r) for r in g["dec"].tolist()])
    return int(g["tile_bytes"]), out, header
