"""Writes tests/golden/preamble.npz: what /comms/preamble_correlator of the reference posts.

Run where a C++ compiler and the reference tree are.  A driver of this project's own (DRIVER below) is written into a temporary directory.
It includes digital/PreambleCorrelator.cpp BY PATH from the reference tree, is compiled against the stand-in framework of
tests/golden/standin (this project's own) with the oracle's flags, and calls the real setPreamble(), setThreshold() and work().  Nothing
compiled and no text of the reference is kept: the file holds parameters and recorded outputs only.  No test reads the reference tree.

Shapes come from the correlator kernel's tile of 4096 positions and its halo of 1024 symbols (pcx_preamble_get_geometry), recorded as
`tile` and `halo`; the GPU suite fails when the library reports another tile.

Cases (unpacked by preamble_model.golden_cases):
  grid/P<P>/w<width>       P in LENGTHS (1027 is beyond the halo: the byte plan), symbol widths 1 and 8; 3 * 4096 + 2 P + 37 symbols of the
                           base array of that width, the preamble planted at the first and the last position, across both seams, in front
                           of a seam and behind one; thresholds 0, 1, P, 8 P - 1, 8 P
  fill/P<P>/<pre>/<fill>   all-zero and all-0xFF input against a random, an all-zero and an all-0xFF preamble, P in 6, 64, 257
  planes/w<w>/P<P>/<lo|hi>[/noisy]   preambles of 1, 2, 4, 8 bit planes at the bottom and at the top of the byte, and the same stream with
                           one bit flipped at each end of a byte inside a planted preamble
  dirty/<clean|dirty>      a bit preamble of 24 against bits and against the same bits with 0x80 set, thresholds 0, P - 1, P
  cuts/P<P>                30000 bits handed to work() in cuts shorter than, equal to and longer than the preamble; the driver keeps the
                           unconsumed tail in front of the next cut, as the circular buffer does; one row per call
Arrays: base1 and base8 (the seeded symbols every stream is cut from), names, spec (one row per case, SPEC_COLUMNS), pre_all and at_all
(preambles and planted positions, one after another), calls (one row per work() call, CALL_COLUMNS) and label_delta: the label indices
of every call one after another, each call's as first differences (the first against 0), which is what makes the calls where every
position matches small.

    python tests/golden/make_preamble_golden.py [--reference /root/reference] [--out tests/golden/preamble.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import preamble_model as M  # noqa: E402

TILE, HALO = 4096, 1024
LENGTHS = [1, 2, 6, 31, 32, 33, 64, 65, 255, 1024, 1027]

DRIVER = r"""
// driver <preamble.bin> <stream.bin> shots <threshold>...       one work() on the whole stream per threshold
// driver <preamble.bin> <stream.bin> cuts <threshold> <cut>...  the stream handed over cut by cut, the unconsumed tail kept
// prints per work() call: "call <threshold> <elements handed> <consumed> <reserve> <elements forwarded> <labels>" and the label indices
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <Pothos/Framework.hpp>
#include "digital/PreambleCorrelator.cpp"

static std::vector<unsigned char> slurp(const char *path)
{
    std::vector<unsigned char> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

static size_t call(PreambleCorrelator &blk, unsigned threshold, const std::vector<unsigned char> &buf)
{
    blk.give(buf.data(), buf.size(), std::vector<Pothos::Label>());
    blk.work();
    const auto &out = blk.out;
    if (out.bytes.size() != blk.in.consumed) std::exit(4);                 // what is forwarded is what is consumed
    for (size_t i = 0; i < out.bytes.size(); i++) if (out.bytes[i] != buf[i]) std::exit(5);
    std::printf("call %u %zu %zu %zu %zu %zu\n", threshold, buf.size(), blk.in.consumed, blk.in.reserve, out.bytes.size(), out.posted.size());
    for (const auto &l : out.posted)
    {
        if (l.id != "sof" or l.width != 1 or l.data.kind != Pothos::Object::NOTHING) std::exit(6);
        std::printf("%llu ", l.index);
    }
    std::printf("\n");
    return blk.in.consumed;
}

int main(int argc, char **a)
{
    if (argc < 5) return 1;
    const auto pre = slurp(a[1]);
    const auto stream = slurp(a[2]);
    const std::string mode = a[3];
    PreambleCorrelator blk;
    blk.setFrameStartId("sof");
    blk.setPreamble(pre);
    if (mode == "shots")
    {
        for (int i = 4; i < argc; i++)
        {
            const unsigned thr = unsigned(std::strtoul(a[i], 0, 10));
            blk.setThreshold(thr);
            call(blk, thr, stream);
        }
        return 0;
    }
    if (mode != "cuts") return 1;
    const unsigned thr = unsigned(std::strtoul(a[4], 0, 10));
    blk.setThreshold(thr);
    std::vector<unsigned char> held;
    size_t at = 0;
    for (int i = 5; i < argc; i++)
    {
        const size_t c = std::strtoull(a[i], 0, 10);
        if (at + c > stream.size()) return 3;
        held.insert(held.end(), stream.begin() + at, stream.begin() + at + c);
        at += c;
        const size_t consumed = call(blk, thr, held);
        held.erase(held.begin(), held.begin() + consumed);
    }
    return 0;
}
"""

# the oracle's flags (oracle/Makefile)
FLAGS = ["-std=c++11", "-O3", "-ffp-contract=off", "-fno-fast-math", "-w"]


def seam_positions(P, n):
    """as seam_stream of tests/test_preamble_gpu.py, but the plant at the first seam straddles it for P = 2 as well"""
    at = [0, TILE - max(P // 2, 1), 2 * TILE - 1, n - P - 1]
    if P < TILE // 4:
        at += [TILE + 1 + P, 2 * TILE - P - 1 - P, 3 * TILE]
    return at


def cases():
    """(name, base width or 0 for a constant stream, n, fill, or-mask, flip position or -1, flip xor, preamble, planted positions,
    thresholds, cuts or None)"""
    out = []
    for P in LENGTHS:
        for width in (1, 8):
            rng = np.random.default_rng(1000 * width + P)
            pre = rng.integers(0, 1 << width, P, dtype=np.uint8)
            pre[0] |= 1
            n = 3 * TILE + 2 * P + 37
            out.append(("grid/P%d/w%d" % (P, width), width, n, 0, 0, -1, 0, pre, seam_positions(P, n), sorted({0, 1, P, 8 * P - 1, 8 * P}), None))
    rng = np.random.default_rng(5)
    for P in (6, 64, 257):
        for pname, pre in (("random", rng.integers(0, 256, P, dtype=np.uint8)), ("zero", np.zeros(P, np.uint8)), ("ones", np.full(P, 0xFF, np.uint8))):
            for fill in (0x00, 0xFF):
                d0 = int(M.POP8[pre ^ np.uint8(fill)].sum())
                out.append(("fill/P%d/%s/%02x" % (P, pname, fill), 0, 2 * TILE + P + 3, fill, 0, -1, 0, pre, [], sorted({0, max(d0 - 1, 0), d0, 8 * P}), None))
    for width in (1, 2, 4, 8):
        rng = np.random.default_rng(40 + width)
        for P in (16, 100):
            for where, shift in (("lo", 0), ("hi", 8 - width)):
                pre = (rng.integers(0, 1 << width, P, dtype=np.uint8) << shift).astype(np.uint8)
                pre[:width] |= ((1 << np.arange(width)) << shift).astype(np.uint8)
                n = 2 * TILE + 500
                at = [7, TILE - 5, n - 1 - P]
                name = "planes/w%d/P%d/%s" % (width, P, where)
                out.append((name, 8, n, 0, 0, -1, 0, pre, at, [0, 1, 2, 3 * P], None))
                out.append((name + "/noisy", 8, n, 0, 0, TILE - 5 + 3, 0x81, pre, at, [0, 1, 2], None))
    rng = np.random.default_rng(3)
    pre = rng.integers(0, 2, 24, dtype=np.uint8)
    pre[0] = 1
    for name, mask in (("clean", 0), ("dirty", 0x80)):
        out.append(("dirty/" + name, 1, 9000, 0, mask, -1, 0, pre, [100, 4090, 8000], [0, 23, 24], None))
    for P in (6, 64, 200):
        rng = np.random.default_rng(60 + P)
        pre = rng.integers(0, 2, P, dtype=np.uint8)
        pre[0] = pre[-1] = 1
        n = 30000
        cuts = [1, P - 1, P, P, P + 1, 1, 2 * P, 5000, 3, 8192, P]
        cuts.append(n - sum(cuts))
        out.append(("cuts/P%d" % P, 1, n, 0, 0, -1, 0, pre, [0, 4096 - P // 2, 9000, 9000 + P, 20000 - 1, n - P - 1], [1], cuts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "preamble.npz"))
    args = ap.parse_args()
    base = {1: np.random.default_rng(20261018).integers(0, 2, 30000, dtype=np.uint8),
            8: np.random.default_rng(20261019).integers(0, 256, 3 * TILE + 2 * max(LENGTHS) + 37, dtype=np.uint8)}
    names, spec, pre_all, at_all, calls, deltas = [], [], [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "standin"), "-I" + args.reference, src, "-o", exe])
        fpre, fx = os.path.join(tmp, "pre.bin"), os.path.join(tmp, "x.bin")
        for name, width, n, fill, mask, flip_at, flip_xor, pre, at, thr, cuts in cases():
            x = M.golden_stream(base, width, n, fill, mask, flip_at, flip_xor, pre, at)
            pre.tofile(fpre)
            x.tofile(fx)
            argv = ["cuts", thr[0]] + cuts if cuts else ["shots"] + thr
            lines = subprocess.check_output([exe, fpre, fx] + [str(v) for v in argv]).decode().splitlines()
            assert len(lines) == 2 * (len(cuts) if cuts else len(thr)), name
            spec.append([width, n, fill, mask, flip_at, flip_xor, sum(p.size for p in pre_all), pre.size, sum(len(a) for a in at_all), len(at),
                         len(calls), len(lines) // 2, int(bool(cuts))])
            names.append(name)
            pre_all.append(pre)
            at_all.append(np.array(at, np.int64))
            for head, body in zip(lines[0::2], lines[1::2]):
                f = head.split()
                assert f[0] == "call"
                idx = np.array([int(v) for v in body.split()], np.int64)
                assert idx.size == int(f[6]) and (idx.size == 0 or (np.diff(idx) > 0).all() and idx[-1] < 1 << 31), name
                calls.append([int(v) for v in f[1:6]] + [sum(d.size for d in deltas), idx.size])
                deltas.append(np.diff(idx, prepend=0).astype(np.uint32))
    data = dict(tile=np.array(TILE), halo=np.array(HALO), base1=base[1], base8=base[8], names=np.array(names), spec=np.array(spec, np.int64),
                pre_all=np.concatenate(pre_all), at_all=np.concatenate(at_all), calls=np.array(calls, np.int64), label_delta=np.concatenate(deltas))
    np.savez_compressed(args.out, **data)
    print("%s: %d cases, %d work() calls, %d labels, %d bytes" % (args.out, len(names), len(calls), data["label_delta"].size, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
