"""Writes tests/golden/scrambler.npz: /comms/scrambler's and /comms/descrambler's outputs as the reference computes them.

Run where the reference tree exists.  A small driver of this project's own (DRIVER below) is compiled with the oracle's flags
(g++ -O3, no -march) against the reference's digital/lfsr.h (GLFSR_init, GLFSR_next) and restates the two blocks' loops: the
constructor's memset, setMode and setPoly(0x19), then the calls of a case.  Nothing compiled is kept.

Cases: both blocks x both modes x the (polynomial, seed) pairs of CONFIGS.  Every case runs the same N random bytes (so the upper
bits of an input byte are exercised) through work() calls cut at CUTS, with setSeed after the third call and setPoly after the
fourth (tests/scrambler_model.py case_ops).  Recorded per case: the output bits (packed), the final data and mask, and the
configuration with the plan the port is to choose for it.

    python tests/golden/make_scrambler_golden.py [--out tests/golden/scrambler.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("PCX_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import scrambler_model as M  # noqa: E402

N = 1000
CUTS = [1, 37, 100, 11, 851]
# name, polynomial set first (a retained mask) or None, polynomial, seed, SERIAL?
CONFIGS = [
    ("default", None, 0x19, 1, 0),
    ("p19_sF", None, 0x19, 0xF, 0),
    ("p7_s1", None, 0x7, 1, 0),
    ("p11021_sACE1", None, 0x11021, 0xACE1, 0),
    ("p80000D_s2A5A5A", None, 0x80000D, 0x2A5A5A, 0),
    ("pbit63_s1234567", None, 0x8000000000000003, 0x1234567, 0),
    ("p19_s10", None, 0x19, 0x10, 1),                    # the seed at 2^m
    ("p19_sF3", None, 0x19, 0xF3, 1),                    # above it
    ("p19_sneg1", None, 0x19, -1, 1),
    ("p1_after_p19", 0x19, 1, 1, 1),                     # the mask of 0x19 kept, polynomial 1
    ("p0_after_p11021", 0x11021, 0, 1, 1),
]

DRIVER = r"""
// driver <descramble> <in.bin> <out.bin> <n> { m <0|1> | p <poly> | s <seed> | w <count> }...
// prints the final data and mask.  The block loops of Scrambler.cpp / Descrambler.cpp over lfsr.h, call by call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lfsr.h"

int main(int argc, char **argv)
{
    if (argc < 5) return 1;
    const int descramble = std::atoi(argv[1]);
    const size_t n = std::strtoull(argv[4], 0, 10);
    std::vector<unsigned char> in(n), out;
    FILE *f = std::fopen(argv[2], "rb");
    if (!f || std::fread(in.data(), 1, n, f) != n) return 2;
    std::fclose(f);
    lfsr_t lfsr;
    lfsr_data_t polynom = 1, seed = 1;
    std::memset(&lfsr, 0, sizeof(lfsr));
    int mult = 1;
    polynom = 0x19;
    GLFSR_init(&lfsr, polynom, seed);
    size_t pos = 0;
    for (int a = 5; a + 1 < argc; a += 2) {
        const char op = argv[a][0];
        if (op == 'm') mult = std::atoi(argv[a + 1]);
        else if (op == 'p') { polynom = (lfsr_data_t)std::strtoull(argv[a + 1], 0, 10); GLFSR_init(&lfsr, polynom, seed); }
        else if (op == 's') { seed = (lfsr_data_t)std::strtoull(argv[a + 1], 0, 10); GLFSR_init(&lfsr, polynom, seed); }
        else if (op == 'w') {
            const size_t c = std::strtoull(argv[a + 1], 0, 10);
            if (pos + c > n) return 4;
            for (size_t i = 0; i < c; i++) {
                const unsigned char b = in[pos + i] & 0x1;
                const unsigned char ret = GLFSR_next(&lfsr);
                const unsigned char o = b ^ ret;
                if (mult) {
                    lfsr.data &= ~lfsr_data_t(0x1);
                    lfsr.data |= descramble ? b : o;
                }
                out.push_back(o);
            }
            pos += c;
        } else return 1;
    }
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 3;
    std::fclose(f);
    std::printf("%llu %llu\n", (unsigned long long)lfsr.data, (unsigned long long)lfsr.mask);
    return 0;
}
"""


def build_driver(workdir):
    src = os.path.join(workdir, "scr_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(workdir, "scr_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fno-fast-math", "-I" + os.path.join(REF, "digital"), src, "-o", exe])
    return exe


def run_driver(exe, workdir, cfg, x):
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    x.tofile(fin)
    args = [exe, str(int(cfg[0])), fin, fout, str(x.shape[0])]
    for op, v in M.case_ops(cfg, CUTS):
        if op == "mode":
            args += ["m", "1" if v == "multiplicative" else "0"]
        elif op == "work":
            args += ["w", str(v)]
        else:
            args += [op[0], str(M.u64(v))]
    data, mask = subprocess.check_output(args, text=True).split()
    out = np.fromfile(fout, dtype=np.uint8)
    assert out.shape[0] == x.shape[0] and out.max() <= 1
    return out, int(data), int(mask)


def i64(v):
    v = M.u64(v)
    return v - (1 << 64) if v >= (1 << 63) else v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "scrambler.npz"))
    a = ap.parse_args()
    if not os.path.isdir(REF):
        sys.exit("the reference tree is not here: nothing to record")
    assert sum(CUTS) == N
    x = np.random.default_rng(20261016).integers(0, 256, N, dtype=np.uint8)
    arrays = {"cuts": np.array(CUTS), "in": x}
    names = []
    with tempfile.TemporaryDirectory() as wd:
        exe = build_driver(wd)
        for descramble in (0, 1):
            for mode in (0, 1):
                for name, pre, poly, seed, serial in CONFIGS:
                    key = "%s/%s/%s" % ("descrambler" if descramble else "scrambler", "multiplicative" if mode else "additive", name)
                    cfg = np.array([descramble, mode, pre is not None, i64(pre or 0), i64(poly), i64(seed), serial], dtype=np.int64)
                    out, data, mask = run_driver(exe, wd, cfg, x)
                    names.append(key)
                    arrays["cfg/" + key] = cfg
                    arrays["out/" + key] = np.packbits(out)
                    arrays["state/" + key] = np.array([data, mask], dtype=np.uint64)
    arrays["cases"] = np.array(names)
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d cases, %d bytes" % (a.out, len(names), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
