"""Writes tests/golden/logic.npz: what the plain C++ operators give that the reference's comparator, bitwise, byte-order and
const-arithmetic loops apply (math/Comparator.cpp, math/ConstComparator.cpp, math/ConstArithmetic.cpp, digital/Bitwise.cpp,
digital/ByteOrder.hpp).

A small driver of this project's own (DRIVER below) is compiled with the oracle's flags (g++ -O3 -ffp-contract=off, no -march) and
applies, element by element, `a OP b` for the six comparisons, `~ & | ^`, `<<` and `>>` by every shift size of the type, the reversal
of a scalar's bytes, and `+ - * /` on T and std::complex<T>.  A constant operand is the same operator with one side broadcast, which
is what this script hands the driver.  Nothing compiled is kept.

Inputs, per type: for the integers MIN, MAX, 0, -1 (MAX again for the unsigned types), their neighbours and seeded noise; for the
comparisons of the float types also NaN, +-inf, +-0.0, the largest and the smallest normal numbers.  The arithmetic inputs of the
float types are finite, with +-0.0 among them and, for the real types, +-inf where the operation meets a finite non-zero constant:
the operators are arith.hip's, which promises the reference's bits for finite operands, and which bits a NaN carries that an
operation CREATES (inf - inf, 0 * inf) is the processor's choice, not the operator's (that a NaN INPUT stays a NaN and leaves its
neighbours alone is checked by tests/test_logic_gpu.py on NaN-ness, not recorded here).  Zero divisors are left out (the reference
traps on them), and so is MIN / -1; a complex integer divisor counts as zero when its norm narrows to zero in the element type,
which is what libstdc++'s operator/= divides by.

The const-arithmetic vectors of the reference's own test (math/TestArithmeticBlocks.cpp:424-508: 100 elements counted up from 2
resp. 1, shifted down by 50 for the signed real types, zeros moved to 1, with the constants 2, 3+2i, 102 and 102+101i) are rebuilt here as
data and run through the same driver.

    python tests/golden/make_logic_golden.py [--out tests/golden/logic.npz]
"""
import argparse
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

TYPES = [("float64", 0, np.float64), ("float32", 1, np.float32), ("int64", 2, np.int64), ("int32", 3, np.int32), ("int16", 4, np.int16),
         ("int8", 5, np.int8), ("uint64", 6, np.uint64), ("uint32", 7, np.uint32), ("uint16", 8, np.uint16), ("uint8", 9, np.uint8)]
CMP = ["GT", "LT", "GE", "LE", "EQ", "NE"]                      # the order of pcx_cmp_op
ARITHK = ["ADDK", "SUBK", "KSUB", "MULK", "DIVK", "KDIV"]       # X+K X-K K-X X*K X/K K/X: the order of pcx_arithk_op
N_CMP, N_BIT, N_SHIFT, N_ARITH, N_REF = 200, 200, 40, 200, 100

DRIVER = r"""
// driver <kind> <scalar> <complex> <n> <in.bin> <out.bin>
//   cmp    in: a[n] b[n]          out: six rows of n bytes, a > b, a < b, a >= b, a <= b, a == b, a != b
//   bit    in: a[n] b[n]          out: ~a, a & b, a | b, a ^ b
//   shift  in: a[n]               out: a << s for s = 0 .. bits - 1, then a >> s
//   swap   in: a[n]               out: every element with its bytes reversed
//   add sub mul div   in: a[n] b[n] (complex: n elements of two scalars)   out: a OP b
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

template <typename E>
static bool load(const char *path, std::vector<E> &a, std::vector<E> *b)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    bool ok = std::fread(a.data(), sizeof(E), a.size(), f) == a.size();
    if (ok && b) ok = std::fread(b->data(), sizeof(E), b->size(), f) == b->size();
    std::fclose(f);
    return ok;
}
template <typename E>
static int save(const char *path, const std::vector<E> &o)
{
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(o.data(), sizeof(E), o.size(), f) != o.size()) return 3;
    std::fclose(f);
    return 0;
}
template <typename E>
static int arith(const std::string &kind, size_t n, const char *fin, const char *fout)
{
    std::vector<E> a(n), b(n), o(n);
    if (!load(fin, a, &b)) return 2;
    for (size_t i = 0; i < n; i++) {
        if (kind == "add") o[i] = a[i] + b[i];
        else if (kind == "sub") o[i] = a[i] - b[i];
        else if (kind == "mul") o[i] = a[i] * b[i];
        else o[i] = a[i] / b[i];
    }
    return save(fout, o);
}
template <typename T>
static typename std::enable_if<std::is_integral<T>::value, int>::type bits(const std::string &kind, size_t n, const char *fin, const char *fout)
{
    std::vector<T> a(n), b(n), o;
    if (kind == "bit") {
        if (!load(fin, a, &b)) return 2;
        for (size_t i = 0; i < n; i++) o.push_back(~a[i]);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] & b[i]);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] | b[i]);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] ^ b[i]);
    } else if (kind == "shift") {
        if (!load<T>(fin, a, nullptr)) return 2;
        for (size_t s = 0; s < 8 * sizeof(T); s++)
            for (size_t i = 0; i < n; i++) o.push_back(a[i] << s);
        for (size_t s = 0; s < 8 * sizeof(T); s++)
            for (size_t i = 0; i < n; i++) o.push_back(a[i] >> s);
    } else {
        if (!load<T>(fin, a, nullptr)) return 2;
        for (size_t i = 0; i < n; i++) {
            unsigned char raw[sizeof(T)], rev[sizeof(T)];
            std::memcpy(raw, &a[i], sizeof(T));
            for (size_t q = 0; q < sizeof(T); q++) rev[q] = raw[sizeof(T) - 1 - q];
            T t;
            std::memcpy(&t, rev, sizeof(T));
            o.push_back(t);
        }
    }
    return save(fout, o);
}
template <typename T>
static typename std::enable_if<!std::is_integral<T>::value, int>::type bits(const std::string &, size_t, const char *, const char *) { return 1; }

template <typename T>
static int run(const std::string &kind, bool cplx, size_t n, const char *fin, const char *fout)
{
    if (kind == "cmp") {
        std::vector<T> a(n), b(n);
        if (!load(fin, a, &b)) return 2;
        std::vector<unsigned char> o;
        for (size_t i = 0; i < n; i++) o.push_back(a[i] > b[i] ? 1 : 0);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] < b[i] ? 1 : 0);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] >= b[i] ? 1 : 0);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] <= b[i] ? 1 : 0);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] == b[i] ? 1 : 0);
        for (size_t i = 0; i < n; i++) o.push_back(a[i] != b[i] ? 1 : 0);
        return save(fout, o);
    }
    if (kind == "bit" || kind == "shift" || kind == "swap") return bits<T>(kind, n, fin, fout);
    if (kind == "add" || kind == "sub" || kind == "mul" || kind == "div")
        return cplx ? arith<std::complex<T>>(kind, n, fin, fout) : arith<T>(kind, n, fin, fout);
    return 1;
}
int main(int argc, char **argv)
{
    if (argc != 7) return 1;
    const std::string kind = argv[1];
    const int s = std::atoi(argv[2]);
    const bool cplx = std::atoi(argv[3]) != 0;
    const size_t n = std::strtoull(argv[4], 0, 10);
    switch (s) {
    case 0: return run<double>(kind, cplx, n, argv[5], argv[6]);
    case 1: return run<float>(kind, cplx, n, argv[5], argv[6]);
    case 2: return run<int64_t>(kind, cplx, n, argv[5], argv[6]);
    case 3: return run<int32_t>(kind, cplx, n, argv[5], argv[6]);
    case 4: return run<int16_t>(kind, cplx, n, argv[5], argv[6]);
    case 5: return run<int8_t>(kind, cplx, n, argv[5], argv[6]);
    case 6: return run<uint64_t>(kind, cplx, n, argv[5], argv[6]);
    case 7: return run<uint32_t>(kind, cplx, n, argv[5], argv[6]);
    case 8: return run<uint16_t>(kind, cplx, n, argv[5], argv[6]);
    case 9: return run<uint8_t>(kind, cplx, n, argv[5], argv[6]);
    }
    return 1;
}
"""


def build_driver(workdir):
    src = os.path.join(workdir, "logic_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(workdir, "logic_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", src, "-o", exe])
    return exe


class Driver:
    def __init__(self, workdir):
        self.wd = workdir
        self.exe = build_driver(workdir)

    def __call__(self, kind, scalar, cplx, n, ins, out_dtype):
        fin, fout = os.path.join(self.wd, "in.bin"), os.path.join(self.wd, "out.bin")
        with open(fin, "wb") as f:
            for a in ins:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([self.exe, kind, str(scalar), str(int(cplx)), str(n), fin, fout])
        return np.fromfile(fout, dtype=out_dtype)


def specials(np_t, floats_special):
    np_t = np.dtype(np_t)
    if np_t.kind == "f":
        fi = np.finfo(np_t)
        v = [0.0, -0.0, 1.0, -1.0, 2.5, -2.5, 3.0, 100.0, -100.0]
        if floats_special:
            v += [np.nan, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny]
        return np.array(v, dtype=np_t)
    info = np.iinfo(np_t)
    return np.array([info.min, info.max, 0, info.max if info.min == 0 else -1, 1, 2, 3, info.min + 1, info.max - 1, info.max // 2, info.max // 2 + 1],
                    dtype=np_t)


def mixed(rng, np_t, n, floats_special=True):
    """the special values first, every one of them, then a mix of them, of small values that meet each other, and of noise"""
    np_t = np.dtype(np_t)
    sp = specials(np_t, floats_special)
    if np_t.kind == "f":
        noise = (rng.standard_normal(n) * 50).astype(np_t)
        small = rng.integers(-3, 4, n).astype(np_t)
    else:
        info = np.iinfo(np_t)
        noise = rng.integers(info.min, info.max, n, dtype=np_t, endpoint=True)
        small = rng.integers(0 if info.min == 0 else -3, 4, n).astype(np_t)
    pick = rng.integers(0, 3, n)
    x = np.where(pick == 0, rng.choice(sp, n), np.where(pick == 1, small, noise)).astype(np_t)
    x[:sp.size] = sp
    return x


def narrowed_norm_is_zero(z, np_t):
    """complex integers: norm(z) narrowed to the element type, the number libstdc++'s operator/= divides by"""
    with np.errstate(over="ignore"):
        w = z.astype(np.int64) if np.dtype(np_t).itemsize < 8 else z
        return (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]).astype(np_t) == 0


def usable_divisors(x, np_t, cplx):
    """x with every element that is a zero divisor, or that sits beside MIN with a -1, replaced by 3 (complex: 3+2i)"""
    np_t = np.dtype(np_t)
    x = x.copy()
    if np_t.kind == "f":
        bad = (x == 0).any(axis=1) if cplx else x == 0
    elif cplx:
        bad = narrowed_norm_is_zero(x, np_t)
    else:
        bad = x == 0
        if np_t.kind == "i":
            bad |= x == -1
    if cplx:
        x[bad] = np.array([3, 2], np_t)
    else:
        x[bad] = 3
    return x


def arith_const_case(drv, scalar, np_t, cplx, x, xd, k):
    """the six operations on x (xd where x divides), one operand the constant k"""
    shape = x.shape
    kb = np.broadcast_to(k, shape)
    n = shape[0]
    out = {}
    for name, kind, a, b in (("ADDK", "add", x, kb), ("SUBK", "sub", x, kb), ("KSUB", "sub", kb, x), ("MULK", "mul", x, kb), ("DIVK", "div", x, kb),
                             ("KDIV", "div", kb, xd)):
        out[name] = drv(kind, scalar, cplx, n, [a, b], np_t).reshape(shape)
    return out


def reference_test_inputs(np_t, cplx, first):
    """math/TestArithmeticBlocks.cpp:451-456 resp. :493-500: elem + first, minus 50 for the signed real types (std::is_signed is false for
    a std::complex), zeros moved to 1 (complex: both parts)"""
    np_t = np.dtype(np_t)
    v = (np.arange(N_REF) + first).astype(np_t)
    if np_t.kind != "u" and not cplx:
        v = (v - np.array(N_REF // 2, np_t)).astype(np_t)
    if cplx:
        v = np.stack([v, np.zeros_like(v)], axis=1)
    v[v == 0] = 1
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "logic.npz"))
    a = ap.parse_args()
    arrays = {}
    with tempfile.TemporaryDirectory() as wd:
        drv = Driver(wd)
        for ti, (name, scalar, np_t) in enumerate(TYPES):
            rng = np.random.default_rng(7000 + ti)
            kind = np.dtype(np_t).kind
            # ---- comparisons: two streams, and a stream against constants
            x, y = mixed(rng, np_t, N_CMP), mixed(rng, np_t, N_CMP)
            y[:N_CMP // 2] = rng.permutation(y[:N_CMP // 2])
            y[-20:] = x[-20:]
            rows = drv("cmp", scalar, False, N_CMP, [x, y], np.uint8).reshape(6, N_CMP)
            arrays["cmp/%s/a" % name], arrays["cmp/%s/b" % name] = x, y
            for op, row in zip(CMP, rows):
                arrays["cmp/%s/%s" % (name, op)] = row
            consts = [0.0, np.nan, -2.5] if kind == "f" else [0, 3, np.iinfo(np_t).max if kind == "u" else -1, np.iinfo(np_t).min]
            for ci, k in enumerate(consts):
                k = np.array([k], np_t)
                rows = drv("cmp", scalar, False, N_CMP, [x, np.broadcast_to(k, x.shape)], np.uint8).reshape(6, N_CMP)
                arrays["cmpk/%s/%d/k" % (name, ci)] = k
                for op, row in zip(CMP, rows):
                    arrays["cmpk/%s/%d/%s" % (name, ci, op)] = row
            # ---- bitwise, shifts, byte order: the integer types
            if kind != "f":
                x, y = mixed(rng, np_t, N_BIT), mixed(rng, np_t, N_BIT)
                rows = drv("bit", scalar, False, N_BIT, [x, y], np_t).reshape(4, N_BIT)
                arrays["bit/%s/a" % name], arrays["bit/%s/b" % name] = x, y
                for op, row in zip(["NOT", "AND", "OR", "XOR"], rows):
                    arrays["bit/%s/%s" % (name, op)] = row
                k = np.array([rng.integers(1, np.iinfo(np_t).max, dtype=np_t)], np_t)
                rows = drv("bit", scalar, False, N_BIT, [x, np.broadcast_to(k, x.shape)], np_t).reshape(4, N_BIT)
                arrays["bitk/%s/k" % name] = k
                for op, row in zip(["NOT", "AND", "OR", "XOR"], rows):
                    if op != "NOT":
                        arrays["bitk/%s/%s" % (name, op)] = row
                nbits = 8 * np.dtype(np_t).itemsize
                x = mixed(rng, np_t, N_SHIFT)
                rows = drv("shift", scalar, False, N_SHIFT, [x], np_t).reshape(2, nbits, N_SHIFT)
                arrays["shift/%s/a" % name], arrays["shift/%s/L" % name], arrays["shift/%s/R" % name] = x, rows[0], rows[1]
                if kind == "u" and nbits > 8:
                    x = mixed(rng, np_t, N_BIT)
                    arrays["swap/%d/a" % (nbits // 8)] = x
                    arrays["swap/%d/out" % (nbits // 8)] = drv("swap", scalar, False, N_BIT, [x], np_t)
            # ---- arithmetic with a constant: real and complex
            for cplx in (False, True):
                shape = (N_ARITH, 2) if cplx else (N_ARITH,)
                x = mixed(rng, np_t, N_ARITH * (2 if cplx else 1), floats_special=False).reshape(shape)
                if kind == "f" and not cplx:
                    x[-4:] = [np.inf, -np.inf, np.inf, -np.inf]
                xd = usable_divisors(x, np_t, cplx)
                if kind == "f":
                    k = np.array([2.5, -0.75] if cplx else [-2.5], np_t)
                elif kind == "u":
                    k = np.array([3, 2] if cplx else [5], np_t)
                else:
                    k = np.array([3, -2] if cplx else [-5], np_t)
                key = "ak/%s/%s" % (name, "c" if cplx else "r")
                arrays[key + "/x"], arrays[key + "/xd"], arrays[key + "/k"] = x, xd, k
                for op, row in arith_const_case(drv, scalar, np_t, cplx, x, xd, k).items():
                    arrays["%s/%s" % (key, op)] = row
                # the reference test's own vectors
                key = "ref/%s/%s" % (name, "c" if cplx else "r")
                xk, kx = reference_test_inputs(np_t, cplx, 2), reference_test_inputs(np_t, cplx, 1)
                k1 = np.array([3, 2] if cplx else [2], np_t)
                k2 = np.array([N_REF + 2, N_REF + 1] if cplx else [N_REF + 2], np_t)
                if cplx and kind != "f":
                    assert not narrowed_norm_is_zero(kx, np_t).any() and not narrowed_norm_is_zero(k1.reshape(1, 2), np_t).any()
                by_k = arith_const_case(drv, scalar, np_t, cplx, xk, xk, k1)
                by_x = arith_const_case(drv, scalar, np_t, cplx, kx, kx, k2)
                arrays[key + "/xbyk_x"], arrays[key + "/xbyk_k"], arrays[key + "/kbyx_x"], arrays[key + "/kbyx_k"] = xk, k1, kx, k2
                for op in ("ADDK", "SUBK", "MULK", "DIVK"):
                    arrays["%s/%s" % (key, op)] = by_k[op]
                for op in ("KSUB", "KDIV"):
                    arrays["%s/%s" % (key, op)] = by_x[op]
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (a.out, len(arrays), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
