"""Writes tests/golden/repack.npz: the outputs of /comms/bits_to_symbols, /comms/symbols_to_bits, /comms/bytes_to_symbols and
/comms/symbols_to_bytes as the reference's loops compute them.

Run where a C++ compiler and the reference tree are.  A small driver of this project's own (DRIVER below) is written into a temporary
directory; it includes the reference's digital/SymbolHelpers.hpp BY PATH from the reference tree (the header is free of Pothos) and
calls its eight functions.  It is compiled with the oracle's flags (g++ -O3 -fno-fast-math).  Nothing compiled and no text of the
reference is kept; the file holds inputs and recorded outputs only.  No test reads the reference tree.

Inputs, shared by all cases: `in_full`, 1680 random bytes over 0..255 (1680 = 2 lcm(1..8): whole groups at every width), and
`in_bits`, 1680 values 0 / 1.  Cases are kind/order/width (tests/repack_model.py CASES, 64 of them):
  out/<case>         the conversion of in_full
  out_bits/<case>    the two bit kinds on in_bits (the clean case)
  out_masked/<case>  symbols_to_bytes on in_full masked to the width: what differs from out/<case> is the leak of the unmasked OR

    python tests/golden/make_repack_golden.py [--reference /root/reference] [--out tests/golden/repack.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import repack_model as M  # noqa: E402

N = 1680

DRIVER = r"""
// driver <kind 0..3> <msb 0|1> <width> <in.bin> <out.bin> <n_in> <n_out>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "digital/SymbolHelpers.hpp"

int main(int argc, char **a)
{
    if (argc != 8) return 1;
    const int kind = std::atoi(a[1]), msb = std::atoi(a[2]);
    const size_t width = std::strtoull(a[3], 0, 10), n_in = std::strtoull(a[6], 0, 10), n_out = std::strtoull(a[7], 0, 10);
    std::vector<unsigned char> in(n_in), out(n_out);
    FILE *f = std::fopen(a[4], "rb");
    if (!f || std::fread(in.data(), 1, n_in, f) != n_in) return 2;
    std::fclose(f);
    switch (kind * 2 + msb) {
    case 0: bitsToSymbolsLSBit(width, in.data(), out.data(), n_out); break;       // counts symbols
    case 1: bitsToSymbolsMSBit(width, in.data(), out.data(), n_out); break;
    case 2: symbolsToBitsLSBit(width, in.data(), out.data(), n_in); break;        // counts symbols
    case 3: symbolsToBitsMSBit(width, in.data(), out.data(), n_in); break;
    case 4: bytesToSymbolsLSBit(width, in.data(), out.data(), n_in); break;       // counts bytes
    case 5: bytesToSymbolsMSBit(width, in.data(), out.data(), n_in); break;
    case 6: symbolsToBytesLSBit(width, in.data(), out.data(), n_out); break;      // counts bytes
    case 7: symbolsToBytesMSBit(width, in.data(), out.data(), n_out); break;
    default: return 1;
    }
    f = std::fopen(a[5], "wb");
    if (!f || std::fwrite(out.data(), 1, n_out, f) != n_out) return 3;
    std::fclose(f);
    return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "repack.npz"))
    args = ap.parse_args()
    rng = np.random.default_rng(20261017)
    in_full = rng.integers(0, 256, N, dtype=np.uint8)
    in_bits = rng.integers(0, 2, N, dtype=np.uint8)
    data = {"in_full": in_full, "in_bits": in_bits, "cases": np.array(M.CASES)}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-fno-fast-math", "-I" + args.reference, src, "-o", exe])

        def run(kind, order, w, x):
            n_out = M.out_elems(kind, w, x.size)
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            x.tofile(fin)
            subprocess.check_call([exe, str(M.KINDS.index(kind)), str(int(order == "MSBit")), str(w), fin, fout, str(x.size), str(n_out)])
            y = np.fromfile(fout, dtype=np.uint8)
            assert y.size == n_out
            return y

        for kind in M.KINDS:
            for order in M.ORDERS:
                for w in M.WIDTHS:
                    name = M.case_name(kind, order, w)
                    data["out/" + name] = run(kind, order, w, in_full)
                    if kind in ("bits_to_symbols", "symbols_to_bits"):
                        data["out_bits/" + name] = run(kind, order, w, in_bits)
                    if kind == "symbols_to_bytes":
                        data["out_masked/" + name] = run(kind, order, w, in_full & np.uint8((1 << w) - 1))
    np.savez_compressed(args.out, **data)
    print("%s: %d cases, %d bytes" % (args.out, len(M.CASES), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
