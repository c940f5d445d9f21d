"""Writes tests/golden/framer.npz: what /comms/preamble_framer and /comms/frame_insert of the reference post, and what its header coder
and decoder compute.

Run where a C++ compiler and the reference tree are.  A driver of this project's own (DRIVER below) is written into a temporary directory.
It includes digital/PreambleFramer.cpp and digital/FrameInsert.cpp (and through it digital/FrameHelper.hpp) BY PATH from the reference
tree, is compiled against the stand-in framework of tests/golden/standin (this project's own) with the oracle's flags, and runs one real
work() per case on a fresh block: PreambleFramer, FrameInsert<std::complex<float>> or FrameInsert<std::complex<double>>.  Nothing compiled
and no text of the reference is kept: the file holds parameters and recorded outputs only.  No test reads the reference tree.

Input elements carry their own position (framer_model.golden_input): bytes are 2 + i % 251, complex elements (i, -(i + 0.5)).  A case
records the posted buffers one after another, the posted labels (the place of the input label each is a copy of, its index, width and the
kind of its data) and the consumed count; or, where the stand-in's postBuffer() met a chunk that is not wholly inside the input
(`label.index - consumed` wrapped), the flag `leaves` and nothing else.  The posted elements are kept as `src`: per output element the
input element it equals (first differences per case, the first against 0), -1 where it equals none, and those elements themselves in
lit_<type>, in order.  framer_model.golden_cases puts the bytes together again; this maker checks that they are the recorded ones.

`backward` is this maker's own flag, by a rule that asks no model: walking the labels in front of the end of the input, `passed` is the
furthest element an earlier start label (its index) or end label (its index + width, clipped to the input) has reached; a start label
whose index, or an end label whose index + width, lies in front of `passed` sets the flag.  Those are the cases of DESIGN.md 18, "a head
never runs backwards", where the project knowingly differs.  Every `leaves` case is `backward`.

Cases (SMALL below restates the 15 scenarios of tests/test_framer_cpu.py as labels with ids; that suite checks the two agree):
  small/<type>/<scenario>      40 elements; a byte preamble of 6, complex_float32 [1, -1j, 0.5] of width 3, complex_float64 [1 + 2j] of
                               width 2 (the reference's inserter always writes its header), header id 0xA7
  seam/<type>/...              3 output tiles of 16 KiB and 37 elements (49189, 6181, 3109): the event lists of
                               test_inserts_around_the_tile_seams_and_at_both_ends of tests/test_framer_gpu.py.  Its start, end, start
                               at one index is backward (the end label passes the element on, the second start label sits on it), so the
                               same three labels come once more as start, start, end
  unit/P<plen>                 byte preambles of 1, 15, 16, 17, 33 with starts at every residue of 16
  run64/<where>                a start label on each of 64 consecutive bytes, before the seam and across it
  header/<type>/<last>         label data absent, a string, integers with data * width of 0, 0xFFF, 0xABCD (6283 x 7) and 70000 x 3, against
                               last preamble symbols (1, 0), (0, -2), (-0.0, 3), (0, 0)
  backward/...                 deliberately backward label lists beside small/<type>/end_width_overlaps_later_labels
  edge/...                     a start label exactly where an end label's width has brought the input: not backward
The header code by itself: enc_* (encodeHeaderWord with the checksum of doChecksum() for all 256 ids at six lengths, as words with bit i
the i-th header bit; for ids 0x55 and 0xA7 at every length the SHA-256 over the little-endian 64-bit words) and dec_* (decodeHeaderWord
on words with no, every single and a seeded sample of two flipped bits: the word, then id, length, checksum and error flag).

    python tests/golden/make_framer_golden.py [--reference /root/reference] [--out tests/golden/framer.npz]
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import framer_model as M  # noqa: E402

TILE_BYTES = 16384
TYPES = ["uint8", "complex_float32", "complex_float64"]
ES = {"uint8": 1, "complex_float32": 8, "complex_float64": 16}

DRIVER = r"""
// driver cases <cases.txt> <out.bin>: per case one work() of a fresh block; prints "result <leaves> <consumed> <bytes> <labels>" and per
//   posted label "L <place of the input label> <index> <width> <kind of data>"; the posted bytes go to out.bin one case after another
// driver encode <id> <length>...: one header word per pair     driver encode_all <id>: the words of every length, raw, to stdout
// driver decode <id> <length> <flip mask>...: the encoded word xor the mask, then what decodeHeaderWord makes of it
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <Pothos/Framework.hpp>
#include "digital/PreambleFramer.cpp"
#include "digital/FrameInsert.cpp"

struct Case {
    std::string type, startId, endId;
    size_t n, width, padding, P;
    unsigned headerId;
    std::vector<double> pre;        // bytes, or re im pairs
    std::vector<Pothos::Label> labels;
};

static void element(unsigned char &v, size_t i) { v = (unsigned char)(2 + i % 251); }
template <typename F> static void element(std::complex<F> &v, size_t i) { v = std::complex<F>(F(i), -(F(i) + F(0.5))); }

static void configure(PreambleFramer &b, const Case &c)
{
    std::vector<unsigned char> pre;
    for (double v : c.pre) pre.push_back((unsigned char)v);
    b.setPreamble(pre);
}
template <typename T> static void configure(FrameInsert<T> &b, const Case &c)
{
    std::vector<T> pre;
    for (size_t i = 0; i < c.P; i++) pre.push_back(T(typename T::value_type(c.pre[2 * i]), typename T::value_type(c.pre[2 * i + 1])));
    b.setPreamble(pre);
    b.setHeaderId((unsigned char)c.headerId);
    b.setSymbolWidth(c.width);
}

template <typename Blk, typename T> static void run(const Case &c, FILE *out)
{
    Blk blk;
    configure(blk, c);
    blk.setFrameStartId(c.startId);
    blk.setFrameEndId(c.endId);
    blk.setPaddingSize(c.padding);
    std::vector<T> x(c.n);
    for (size_t i = 0; i < c.n; i++) element(x[i], i);
    blk.give(x.data(), c.n, c.labels);
    bool leaves = false;
    try { blk.work(); } catch (const Pothos::LeavesItsBuffer &) { leaves = true; }
    if (leaves) { std::printf("result 1 0 0 0\n"); return; }
    std::printf("result 0 %zu %zu %zu\n", blk.in.consumed, blk.out.bytes.size(), blk.out.posted.size());
    for (const auto &l : blk.out.posted) std::printf("L %ld %llu %zu %d\n", l.ordinal, l.index, l.width, int(l.data.kind));
    if (std::fwrite(blk.out.bytes.data(), 1, blk.out.bytes.size(), out) != blk.out.bytes.size()) std::exit(3);
}

static uint64_t encode(unsigned id, unsigned length)
{
    FrameHeaderFields f;
    f.id = uint8_t(id);
    f.length = uint16_t(length);
    f.chksum = f.doChecksum();
    char bits[NUM_HEADER_BITS];
    encodeHeaderWord(bits, f);
    uint64_t w = 0;
    for (int i = 0; i < NUM_HEADER_BITS; i++) w |= uint64_t(bits[i] != 0) << i;
    return w;
}

int main(int argc, char **a)
{
    if (argc < 3) return 1;
    const std::string mode = a[1];
    if (mode == "encode")
    {
        for (int i = 2; i + 1 < argc; i += 2) std::printf("%llu\n", (unsigned long long)encode(std::atoi(a[i]), std::atoi(a[i + 1])));
        return 0;
    }
    if (mode == "encode_all")
    {
        for (unsigned len = 0; len < 65536; len++)
        {
            const uint64_t w = encode(std::atoi(a[2]), len);
            unsigned char le[8];
            for (int k = 0; k < 8; k++) le[k] = (unsigned char)(w >> (8 * k));
            std::fwrite(le, 1, 8, stdout);
        }
        return 0;
    }
    if (mode == "decode")
    {
        for (int i = 2; i + 2 < argc; i += 3)
        {
            const uint64_t w = encode(std::atoi(a[i]), std::atoi(a[i + 1])) ^ std::strtoull(a[i + 2], 0, 10);
            char bits[NUM_HEADER_BITS];
            for (int k = 0; k < NUM_HEADER_BITS; k++) bits[k] = char((w >> k) & 1);
            FrameHeaderFields f;
            decodeHeaderWord(bits, f);
            std::printf("%llu %u %u %u %d\n", (unsigned long long)w, unsigned(f.id), unsigned(f.length), unsigned(f.chksum), int(f.error));
        }
        return 0;
    }
    if (mode != "cases" or argc < 4) return 1;
    std::ifstream in(a[2]);
    FILE *out = std::fopen(a[3], "wb");
    if (!in or !out) return 2;
    std::string line, word;
    Case c;
    size_t left = 0;
    bool open = false;
    auto finish = [&]() {
        if (c.type == "uint8") run<PreambleFramer, unsigned char>(c, out);
        else if (c.type == "complex_float32") run<FrameInsert<std::complex<float>>, std::complex<float>>(c, out);
        else if (c.type == "complex_float64") run<FrameInsert<std::complex<double>>, std::complex<double>>(c, out);
        else std::exit(4);
    };
    while (std::getline(in, line))
    {
        std::istringstream s(line);
        s >> word;
        if (word == "case")
        {
            c = Case();
            std::string sid, eid;
            s >> c.type >> c.n >> c.width >> c.headerId >> c.padding >> c.P >> left >> sid >> eid;       // ids behind a '='
            c.startId = sid.substr(1);
            c.endId = eid.substr(1);
            open = true;
        }
        else if (word == "pre")
        {
            std::string v;
            while (s >> v) c.pre.push_back(std::strtod(v.c_str(), 0));
        }
        else if (word == "label")
        {
            std::string id, kind, value;
            unsigned long long index, width;
            s >> id >> index >> width >> kind >> value;
            Pothos::Object data;
            if (kind == "u") data = Pothos::Object(std::strtoull(value.c_str(), 0, 10));
            else if (kind == "s") data = Pothos::Object(value.substr(1));
            c.labels.push_back(Pothos::Label(id.substr(1), data, index, size_t(width)));
            left--;
        }
        else return 5;
        if (open and left == 0 and not c.pre.empty()) { finish(); open = false; }
    }
    std::fclose(out);
    return open ? 6 : 0;
}
"""

# the oracle's flags (oracle/Makefile)
FLAGS = ["-std=c++11", "-O3", "-ffp-contract=off", "-fno-fast-math", "-w"]

S, E = "frameStart", "frameEnd"
# name -> (labels [(id, index, width, data)], padding, start id, end id): the scenarios of tests/test_framer_cpu.py
SMALL = {
    "reference": ([(S, 5, 1, None), (E, 33, 1, None)], 13, S, E),
    "index_0": ([(S, 0, 1, 7), ("tick", 0, 1, None)], 13, S, E),
    "last_element": ([(S, 39, 1, None), (E, 39, 1, None)], 13, S, E),
    "beyond_the_buffer": ([(S, 5, 1, None), (S, 40, 1, None), (E, 77, 1, None)], 13, S, E),
    "start_and_end_at_one_index": ([(S, 7, 1, None), (E, 7, 1, None), ("tick", 9, 1, None)], 13, S, E),
    "end_and_start_at_one_index": ([(E, 7, 1, None), (S, 7, 1, None), ("tick", 9, 1, None)], 13, S, E),
    "two_starts_at_one_index": ([(S, 9, 1, 1), (S, 9, 1, 2), ("tick", 20, 1, None), (E, 21, 1, None)], 13, S, E),
    "end_width_past_the_buffer": ([(E, 30, 100, None)], 13, S, E),
    "end_width_overlaps_later_labels": ([(E, 10, 8, None), (S, 12, 1, 3), ("tick", 14, 1, None), (E, 15, 2, None), (S, 30, 1, None)], 5, S, E),
    "end_width_0": ([(E, 10, 0, None), ("tick", 12, 1, None)], 4, S, E),
    "equal_start_and_end_ids": ([("x", 5, 1, None), ("x", 20, 1, None)], 13, "x", "x"),
    "empty_end_id_with_an_empty_id_label": ([(S, 5, 1, None), ("", 20, 1, None), ("else", 25, 1, None)], 13, S, ""),
    "padding_0": ([(S, 5, 1, None), (E, 33, 1, None), ("tick", 35, 1, None)], 0, S, E),
    "no_labels": ([], 13, S, E),
    "others_only": ([("tick", 0, 1, None), ("tick", 39, 1, None)], 13, S, E),
}
# (preamble, symbol width) per type: the small cases, and the seam cases (SETUP of tests/test_framer_gpu.py)
SMALL_SETUP = {"uint8": ([0, 1, 1, 1, 1, 0], 1), "complex_float32": ([1, -1j, 0.5], 3), "complex_float64": ([1 + 2j], 2)}
SEAM_SETUP = {"uint8": ([0, 1, 1, 1, 1, 0, 1], 1), "complex_float32": ([1, -1, 1j], 3), "complex_float64": ([1, 1, -1 + 0.5j], 2)}


def from_events(events):
    """[(index, width, kind, length)] -> labels; a start label's length travels as its data"""
    ids = {"start": S, "end": E, "other": "tick"}
    return [(ids[k], i, w, (ln if k == "start" and ln else None)) for i, w, k, ln in events]


def cases():
    """[(name, type, n, preamble, symbol width, header id, padding, start id, end id, labels)]"""
    out = []
    for t in TYPES:
        pre, width = SMALL_SETUP[t]
        for name, (labels, padding, sid, eid) in SMALL.items():
            out.append(("small/%s/%s" % (t, name), t, 40, pre, width, 0xA7, padding, sid, eid, labels))
    for t in TYPES:
        pre, width = SEAM_SETUP[t]
        tile = TILE_BYTES // ES[t]
        n = 3 * tile + 37
        P = len(pre) * width + (M.HEADER_BITS if t != "uint8" else 0)
        lists = {}
        for where, at in (("first", 0), ("before_seam", tile - 1), ("seam", tile), ("last", n - 1)):
            lists["start_" + where] = [(at, 1, "start", 0x1234)]
            lists["end_" + where] = [(at, 1, "end", 0)]
            lists["start_end_start_" + where] = [(at, 1, "start", 77), (at, 1, "end", 0), (at, 1, "start", 78)]
            lists["start_start_end_" + where] = [(at, 1, "start", 77), (at, 1, "start", 78), (at, 1, "end", 0)]     # the same three, none backward
        lists["end_reaches_the_end"] = [(n - 9, 9, "end", 0)]
        lists["end_width_2_40"] = [(n - 9, 1 << 40, "end", 0)]
        lists["all_in_one"] = [(0, 1, "start", 1), (tile - 1, 1, "end", 0), (tile, 1, "start", 2), (2 * tile - P - 13, 1, "start", 3), (n - 1, 1, "start", 4),
                               (n - 1, 1, "end", 0)]
        lists["insert_on_an_output_seam"] = [(0, 1, "start", 5), (tile - P, 1, "start", 6)]      # the second insert begins at element `tile` of the output
        for name, events in lists.items():
            out.append(("seam/%s/%s" % (t, name), t, n, pre, width, 0xA7, 13, S, E, from_events(events)))
    tile = TILE_BYTES
    n = 3 * tile + 37
    for plen in (1, 15, 16, 17, 33):
        pre = ((np.arange(plen) * 37 + 11) % 251 + 1).tolist()
        at = [0, 1, 2, 19, 20, 50] + [tile - 40 + 7 * k for k in range(12)] + [2 * tile + 100 + 17 * k for k in range(16)] + [n - 2, n - 1]
        out.append(("unit/P%d" % plen, "uint8", n, pre, 1, 0x55, 3, S, E, from_events([(i, 1, "start", 0) for i in at] + [(n - 1, 1, "end", 0)])))
    for where, i0 in (("before_the_seam", tile - 128 - 5), ("across_the_seam", tile - 61)):
        out.append(("run64/" + where, "uint8", n, [9], 1, 0x55, 0, S, E, from_events([(i0 + k, 1, "start", 0) for k in range(64)])))
    for t in TYPES[1:]:
        for lname, last in (("1_0", (1.0, 0.0)), ("0_m2", (0.0, -2.0)), ("m0_3", (-0.0, 3.0)), ("0_0", (0.0, 0.0))):
            labels = [(S, 3, 1, None), ("note", 3, 1, "hello"), (S, 20, 1, "text"), (S, 50, 1, 0), (S, 90, 1, 0xFFF), (S, 130, 7, 6283), (S, 200, 3, 70000),
                      ("tick", 210, 2, 5), (E, 250, 1, 9), (E, 260, 1, "end")]
            out.append(("header/%s/%s" % (t, lname), t, 300, [(0.5, 0.5), last], 2, 0x55, 4, S, E, labels))
    pre, width = SMALL_SETUP["uint8"]
    for t in TYPES:
        p, w = SMALL_SETUP[t]
        # only end labels: the second ends in front of what the first passed on, and the reference's min() posts the whole remainder
        out.append(("backward/%s/ends_only" % t, t, 40, p, w, 0xA7, 5, S, E, [(E, 10, 8, None), (E, 12, 2, None), (E, 30, 1, None)]))
    out.append(("backward/uint8/start_behind_an_end", "uint8", 40, pre, width, 0xA7, 5, S, E, [(E, 10, 8, None), (S, 17, 1, None)]))
    out.append(("edge/uint8/start_where_an_end_stands", "uint8", 40, pre, width, 0xA7, 5, S, E, [(E, 10, 8, None), (S, 18, 1, None), ("tick", 11, 1, None)]))
    out.append(("backward/uint8/end_ends_in_front_of_a_start", "uint8", 40, pre, width, 0xA7, 5, S, E, [(S, 20, 1, None), (E, 10, 5, None), (S, 30, 1, None)]))
    return out


def is_backward(n, labels, sid, eid):
    passed = 0
    flag = False
    for lid, index, width, _ in labels:
        if index >= n:
            continue
        if lid == sid:
            flag |= index < passed
            passed = max(passed, index)
        elif lid == eid:
            flag |= index + width < passed
            passed = max(passed, min(index + width, n))
    return flag


def pre_pairs(pre):
    """complex symbols or (re, im) pairs -> [(re, im)] of floats, a negative zero kept"""
    return [(float(p[0]), float(p[1])) if isinstance(p, tuple) else (float(complex(p).real), float(complex(p).imag)) for p in pre]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "framer.npz"))
    args = ap.parse_args()
    todo = cases()
    text = []
    for name, t, n, pre, width, hid, padding, sid, eid, labels in todo:
        assert all(index < 1 << 31 for _, index, _, _ in labels), name
        text.append("case %s %d %d %d %d %d %d =%s =%s" % (t, n, width, hid, padding, len(pre), len(labels), sid, eid))
        text.append("pre " + (" ".join(str(int(v)) for v in pre) if t == "uint8" else " ".join("%r %r" % p for p in pre_pairs(pre))))
        for lid, index, w, data in labels:
            kind, value = ("n", "-") if data is None else ("u", str(data)) if isinstance(data, int) else ("s", "=" + data)
            text.append("label =%s %d %d %s %s" % (lid, index, w, kind, value))
    rng = np.random.default_rng(20261018)
    enc_pairs = [(i, ln) for ln in (0, 1, 0x0FFF, 0x1000, 0xABCD, 0xFFFF) for i in range(256)]
    dec_in = []
    for i, ln in ((0x55, 0), (0xA7, 0xABCD), (0x00, 0xFFFF), (0xFF, 0x0FFF), (0x3C, 0x1000), (0x81, 1)):
        dec_in.append((i, ln, 0))
        dec_in += [(i, ln, 1 << k) for k in range(M.HEADER_BITS)]
        for _ in range(60):
            a, b = sorted(rng.choice(M.HEADER_BITS, 2, replace=False).tolist())
            dec_in.append((i, ln, (1 << a) | (1 << b)))
        dec_in += [(i, ln, (1 << (2 + 8 * k)) | (1 << (9 + 8 * k))) for k in range(7)]          # two flips inside every one of the seven words
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "standin"), "-I" + args.reference, src, "-o", exe])
        fcases, fout = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "out.bin")
        open(fcases, "w").write("\n".join(text) + "\n")
        lines = subprocess.check_output([exe, "cases", fcases, fout]).decode().splitlines()
        raw = np.fromfile(fout, np.uint8)
        enc_words = [int(v) for v in subprocess.check_output([exe, "encode"] + [str(v) for p in enc_pairs for v in p]).decode().split()]
        enc_sha = [hashlib.sha256(subprocess.check_output([exe, "encode_all", str(i)])).hexdigest() for i in (0x55, 0xA7)]
        dec_out = [[int(v) for v in ln.split()] for ln in subprocess.check_output([exe, "decode"] + [str(v) for d in dec_in for v in d]).decode().splitlines()]
    assert len(enc_words) == len(enc_pairs) and len(dec_out) == len(dec_in)

    names, rows, sids, eids, pre_u8, pre_c, lab_id, lab_num, lab_text, src_all, posted = [], [], [], [], [], [], [], [], [], [], []
    lit = {t: [] for t in TYPES}
    li = ri = 0
    for name, t, n, pre, width, hid, padding, sid, eid, labels in todo:
        f = lines[li].split()
        assert f[0] == "result", (name, lines[li])
        leaves, consumed, nbytes, nposted = (int(v) for v in f[1:])
        got = [[int(v) for v in ln.split()[1:]] for ln in lines[li + 1:li + 1 + nposted]]
        assert all(ln.startswith("L ") for ln in lines[li + 1:li + 1 + nposted])
        li += 1 + nposted
        out = raw[ri:ri + nbytes].reshape(-1, ES[t])
        ri += nbytes
        backward = is_backward(n, labels, sid, eid)
        assert backward or not leaves, name
        x = M.golden_input(t, n)
        where = {}
        for i in range(n - 1, -1, -1):
            where[x[i].tobytes()] = i
        src = np.array([where.get(r.tobytes(), -1) for r in out], np.int64)
        lits = out[src < 0]
        assert np.array_equal(M.golden_output(x, np.diff(src, prepend=0), lits), out) and (labels or leaves or not lits.size), name
        pre_store = pre_u8 if t == "uint8" else pre_c
        rows.append([TYPES.index(t), n, width, hid, padding, len(pre), len(pre_store), len(lab_id), len(labels), leaves, int(backward), consumed,
                     out.shape[0], sum(s.size for s in src_all), sum(a.shape[0] for a in lit[t]), lits.shape[0], len(posted), nposted])
        names.append(name)
        sids.append(sid)
        eids.append(eid)
        pre_store += [int(v) for v in pre] if t == "uint8" else pre_pairs(pre)
        for lid, index, w, data in labels:
            lab_id.append(lid)
            lab_num.append([index, w, 0 if data is None else 1 if isinstance(data, int) else 2, data if isinstance(data, int) else 0])
            lab_text.append(data if isinstance(data, str) else "")
        src_all.append(np.diff(src, prepend=0).astype(np.int32))
        lit[t].append(lits)
        posted += got
    assert li == len(lines) and ri == raw.size
    data = dict(tile_bytes=np.array(TILE_BYTES), names=np.array(names), case=np.array(rows, np.int64), start_id=np.array(sids), end_id=np.array(eids),
                pre_u8=np.array(pre_u8, np.uint8), pre_c=np.array(pre_c, np.float64).reshape(-1, 2), label_id=np.array(lab_id),
                label_num=np.array(lab_num, np.int64), label_text=np.array(lab_text), src=np.concatenate(src_all),
                posted=np.array(posted, np.int64).reshape(-1, 4), enc_in=np.array(enc_pairs, np.int64), enc_word=np.array(enc_words, np.uint64),
                enc_all_id=np.array([0x55, 0xA7]), enc_all_sha=np.array(enc_sha), dec=np.array(dec_out, np.uint64))
    for t in TYPES:
        data["lit_" + t] = np.concatenate(lit[t])
    np.savez_compressed(args.out, **data)
    print("%s: %d cases (%d backward, %d leave their buffer), %d header words, %d decoded, %d bytes" % (
        args.out, len(names), int(data["case"][:, 10].sum()), int(data["case"][:, 9].sum()), len(enc_words), len(dec_out), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
