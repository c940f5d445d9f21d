"""Writes tests/golden/symbols.npz: the outputs of /comms/symbol_mapper, /comms/symbol_slicer, /comms/differential_encoder and
/comms/differential_decoder as the reference's compiler computes them.

Run where a C++ compiler is.  A small driver of this project's own (DRIVER below) restates the four work() loops of the reference's
digital/ directory for all twelve stream types and is compiled with the oracle's flags (g++ -O3 -fno-fast-math, no -march), so the
slicer's powf(x, 2) becomes the one float product the reference's build has.  Nothing compiled is kept; the file holds inputs, maps and
recorded outputs only.

Cases (tests/symbol_model.py names the types and the coder scenario):
  map/<type>/<len>      map lengths 1, 2, 4, 256, 512, random input bytes (upper bits set)
  slice/<type>/<map>    maps bpsk, qpsk (complex types), rand16, pts256, pts300, dup, and naninf for the float types; inputs: random
                        values, the map's own points, exact ties, doubles that differ below float precision, integers up to 2^30 / 2^62,
                        denormals, infinities, NaN, values whose squared distance overflows float
  enc/<symbols>, dec/<symbols>   the fifteen symbol counts, random bytes 0..255, five work() calls and a setSymbols between two of
                        them; the carried byte and the plan (the 65536-pair check, run by the driver) are recorded

    python tests/golden/make_symbols_golden.py [--out tests/golden/symbols.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import symbol_model as M  # noqa: E402

DRIVER = r"""
// driver map|slice <type> <in.bin> <map.bin> <out.bin> <n> <M>
// driver enc|dec <in.bin> <out.bin> <n> { s <symbols> | w <count> }...      prints the carried byte and the encoder's plan
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

template <typename T>
static std::vector<T> slurp(const char *path, size_t n)
{
    std::vector<T> v(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) std::exit(2);
    std::fclose(f);
    return v;
}
template <typename T>
static void spill(const char *path, const std::vector<T> &v)
{
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3);
    std::fclose(f);
}

template <typename T>
float separation(T a, T b)
{
    return std::abs(b - a);
}
template <typename T>
float separation(std::complex<T> a, std::complex<T> b)
{
    return powf(b.real() - a.real(), 2) + powf(b.imag() - a.imag(), 2);
}

template <typename T>
static int run_map(char **a)
{
    const size_t n = std::strtoull(a[6], 0, 10), len = std::strtoull(a[7], 0, 10);
    const std::vector<unsigned char> in = slurp<unsigned char>(a[3], n);
    const std::vector<T> table = slurp<T>(a[4], len);
    const unsigned int nbits = std::log2(len);
    const unsigned char mask = (1 << nbits) - 1;
    std::vector<T> out(n);
    for (unsigned int i = 0; i < n; i++) out[i] = table[in[i] & mask];
    spill(a[5], out);
    return 0;
}
template <typename T>
static int run_slice(char **a)
{
    const size_t n = std::strtoull(a[6], 0, 10), len = std::strtoull(a[7], 0, 10);
    const std::vector<T> in = slurp<T>(a[3], n);
    const std::vector<T> table = slurp<T>(a[4], len);
    std::vector<unsigned char> out(n);
    for (unsigned int i = 0; i < n; i++) {
        std::pair<unsigned char, float> nearest = std::make_pair(0, FLT_MAX);
        for (unsigned int j = 0; j < table.size(); j++) {
            float d = separation(in[i], table[j]);
            if (d < nearest.second) nearest = std::make_pair(j, d);
        }
        out[i] = nearest.first;
    }
    spill(a[5], out);
    return 0;
}
template <typename T>
static int run_typed(const std::string &kind, bool cplx, char **a)
{
    if (kind == "map") return cplx ? run_map<std::complex<T>>(a) : run_map<T>(a);
    return cplx ? run_slice<std::complex<T>>(a) : run_slice<T>(a);
}

static int run_coder(bool decode, int argc, char **a)
{
    const size_t n = std::strtoull(a[4], 0, 10);
    const std::vector<unsigned char> in = slurp<unsigned char>(a[2], n);
    std::vector<unsigned char> out;
    uint8_t carried = 0;
    uint32_t symbols = 2;
    size_t pos = 0;
    for (int k = 5; k + 1 < argc; k += 2) {
        if (a[k][0] == 's') { symbols = (uint32_t)std::strtoull(a[k + 1], 0, 10); continue; }
        const uint32_t len = (uint32_t)std::strtoull(a[k + 1], 0, 10);
        if (pos + len > n) return 4;
        const uint8_t *p = in.data() + pos;
        uint8_t last = carried;
        for (uint32_t i = 0; i < len; i++) {
            if (decode) {
                const uint8_t before = last;
                last = *p++;
                out.push_back((last - before + symbols) % symbols);
            } else {
                last = (*p++ + last + symbols) % symbols;
                out.push_back(last);
            }
        }
        carried = last;
        pos += len;
    }
    spill(a[3], out);
    // the encoder's step against (in + last) mod min(symbols, 256), all 65536 pairs
    int serial = 0;
    const uint32_t m = symbols < 256 ? symbols : 256;
    for (uint32_t l = 0; l < 256; l++)
        for (uint32_t b = 0; b < 256; b++) {
            const uint8_t step = (uint8_t)((b + l + symbols) % symbols);
            if (step != (uint8_t)((b + l) % m)) serial = 1;
        }
    std::printf("%u %d\n", (unsigned)carried, serial);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 1;
    const std::string kind = argv[1];
    if (kind == "enc" || kind == "dec") return run_coder(kind == "dec", argc, argv);
    if (argc < 8) return 1;
    std::string t = argv[2];
    const bool cplx = t.compare(0, 8, "complex_") == 0;
    if (cplx) t = t.substr(8);
    if (t == "float64") return run_typed<double>(kind, cplx, argv);
    if (t == "float32") return run_typed<float>(kind, cplx, argv);
    if (t == "int64") return run_typed<int64_t>(kind, cplx, argv);
    if (t == "int32") return run_typed<int32_t>(kind, cplx, argv);
    if (t == "int16") return run_typed<int16_t>(kind, cplx, argv);
    if (t == "int8") return run_typed<int8_t>(kind, cplx, argv);
    return 1;
}
"""

NMAP = 300
NRAND = 256
NCODE = sum(M.CODER_CUTS)


def build_driver(workdir):
    src = os.path.join(workdir, "sym_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(workdir, "sym_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-fno-fast-math", src, "-o", exe])
    return exe


def magnitude(scalar):
    """the largest magnitude of a map entry or a sample: no difference leaves the reference's int / long"""
    return {"int64": 2 ** 62 - 1, "int32": 2 ** 30 - 1, "int16": 32767, "int8": 127}.get(scalar, 0)


def points(rng, scalar, cplx, n):
    """n random map entries / samples of a type"""
    shape = (n, 2) if cplx else (n,)
    if scalar.startswith("float"):
        return (rng.standard_normal(shape) * 1.5).astype(scalar)
    big = magnitude(scalar)
    a = rng.integers(-big, big + 1, shape, dtype=np.int64)
    if scalar == "int64":
        a = (a >> 10) << 10         # 52 significant bits: exact as a double, so the case can cross the runner ABI as well
    small = rng.integers(-9, 10, shape, dtype=np.int64)
    return np.where(rng.random(shape) < 0.5, a, small).astype(scalar)


def maps_of(rng, scalar, cplx):
    out = {}
    one = np.array([1], dtype=scalar)[0]
    if cplx:
        out["bpsk"] = np.array([[-1, 0], [1, 0]], dtype=scalar)
        out["qpsk"] = np.array([[-1, -1], [-1, 1], [1, 1], [1, -1]], dtype=scalar)
    else:
        out["bpsk"] = np.array([-one, one], dtype=scalar)
    out["rand16"] = points(rng, scalar, cplx, 16)
    out["pts256"] = points(rng, scalar, cplx, 256)
    out["pts300"] = points(rng, scalar, cplx, 300)
    dup = points(rng, scalar, cplx, 8)
    dup[5] = dup[1]
    dup[6] = dup[0]
    out["dup"] = dup
    if scalar.startswith("float"):
        m = points(rng, scalar, cplx, 8)
        flat = m.reshape(-1)
        flat[0] = np.nan
        flat[3] = np.inf
        flat[5] = -np.inf
        out["naninf"] = m
    return out


def samples_for(rng, scalar, cplx, m):
    """the inputs of one slicer case: random values, the map's points, ties between neighbouring entries and the special values"""
    parts = [points(rng, scalar, cplx, NRAND), m[:24]]
    k = min(m.shape[0] - 1, 12)
    if scalar.startswith("float"):
        with np.errstate(invalid="ignore", over="ignore"):
            parts.append(((m[:k].astype(np.float64) + m[1:k + 1].astype(np.float64)) / 2).astype(scalar))      # midway: exact ties where representable
        sp = [0.0, -0.0, 1e-40, -1e-42, 1e-45, np.inf, -np.inf, np.nan, 1e20, -3e19, 3.3e38, -3.4e38]
        if scalar == "float64":
            sp += [5e-324, 1e-310, 1e200, -1e300, 1.7e308, 1.0 + 1e-12, 1.0 - 1e-13, -1.0 + 1e-15, 1e-60, 3.5e38, 6e38]
        sp = np.array(sp, dtype=scalar)
        if cplx:
            sp = np.stack([sp, np.roll(sp, 3)], axis=1)
            sp = np.concatenate([sp, np.stack([sp[:, 0], np.zeros_like(sp[:, 0])], axis=1)])
        parts.append(sp)
        if scalar == "float64":                                   # within float precision of a map point: the narrowing creates ties
            near = m[:8].copy()
            near = near * (1 + 2.0 ** -40)
            parts.append(near.astype(scalar))
    else:
        wide = m[:k].astype(object) + m[1:k + 1].astype(object)
        parts.append(np.array(wide // 2, dtype=object).astype(scalar))       # midway (exact when the sum is even)
        big = magnitude(scalar)
        sp = np.array([0, 1, -1, 2, -2, big, -big, big - 1, -(big - 1), big // 2 + 1, -(big // 3)], dtype=scalar)
        if cplx:
            sp = np.stack([sp, np.roll(sp, 2)], axis=1)
        parts.append(sp)
    return np.ascontiguousarray(np.concatenate(parts))


def run(exe, wd, kind, tname, x, m):
    fin, fmap, fout = (os.path.join(wd, f) for f in ("in.bin", "map.bin", "out.bin"))
    x.tofile(fin)
    m.tofile(fmap)
    subprocess.check_call([exe, kind, tname, fin, fmap, fout, str(x.shape[0]), str(m.shape[0])])
    if kind == "slice":
        return np.fromfile(fout, dtype=np.uint8)
    return np.fromfile(fout, dtype=m.dtype).reshape((x.shape[0],) + m.shape[1:])


def run_coder(exe, wd, decode, symbols, x):
    fin, fout = os.path.join(wd, "in.bin"), os.path.join(wd, "out.bin")
    x.tofile(fin)
    args = [exe, "dec" if decode else "enc", fin, fout, str(x.shape[0])]
    for op, v in M.coder_ops(symbols):
        args += [op, str(v)]
    last, serial = subprocess.check_output(args, text=True).split()
    return np.fromfile(fout, dtype=np.uint8), int(last), int(serial)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "symbols.npz"))
    a = ap.parse_args()
    rng = np.random.default_rng(20261017)
    arrays, names = {}, []
    bytes_in = rng.integers(0, 256, NMAP, dtype=np.uint8)
    code_in = rng.integers(0, 256, NCODE, dtype=np.uint8)
    arrays["map_in"] = bytes_in
    arrays["code_in"] = code_in
    with tempfile.TemporaryDirectory() as wd:
        exe = build_driver(wd)
        for scalar, cplx in M.TYPES:
            tname = M.type_name(scalar, cplx)
            for length in (1, 2, 4, 256, 512):
                key = "map/%s/%d" % (tname, length)
                m = points(rng, scalar, cplx, length)
                arrays["m/" + key] = m
                arrays["out/" + key] = run(exe, wd, "map", tname, bytes_in, m)
                names.append(key)
            for mname, m in maps_of(rng, scalar, cplx).items():
                key = "slice/%s/%s" % (tname, mname)
                x = samples_for(rng, scalar, cplx, m)
                arrays["m/" + key] = m
                arrays["in/" + key] = x
                arrays["out/" + key] = run(exe, wd, "slice", tname, x, m)
                names.append(key)
        for decode in (0, 1):
            for symbols in M.CODER_SYMBOLS:
                key = "%s/%d" % ("dec" if decode else "enc", symbols)
                out, last, serial = run_coder(exe, wd, decode, symbols, code_in)
                arrays["out/" + key] = out
                arrays["state/" + key] = np.array([last, 0 if decode else serial], dtype=np.int64)
                names.append(key)
    arrays["cases"] = np.array(names)
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d cases, %d bytes" % (a.out, len(names), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
