"""Writes tests/golden/dcremoval.npz: /comms/dc_removal's outputs as the reference computes them.

Run where the reference tree exists.  A small driver of this project's own (DRIVER below) is compiled with g++ -O2 against the
reference's filter/MovingAverage.hpp -- a plain std::deque stands in for Pothos::Util::RingDeque in the build directory -- and
replays DCRemoval::work's loop.  Nothing compiled is kept.

Cases: the 12 element types x average size D in {1, 2, 3, 7, 64, 512} x cascade size C in {1, 2, 3} x three inputs (seeded
random at low amplitude, seeded random at full scale, the alternating full-scale pattern +max, min, +max, ...).  One input stream
per (type, pattern) is stored; a case reads its first n(D) samples.  A configuration whose divisor narrowed to the accumulator
type is zero (the reference dies of SIGFPE there) is recorded as refused.

    python tests/golden/make_dcremoval_golden.py [--out tests/golden/dcremoval.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("PCX_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

# (name, scalar code as include/pcx.h pcx_scalar, numpy scalar, accumulator bits for integers)
TYPES = [("float64", 0, np.float64, 0), ("float32", 1, np.float32, 0), ("int64", 2, np.int64, 64),
         ("int32", 3, np.int32, 64), ("int16", 4, np.int16, 32), ("int8", 5, np.int8, 16)]
DTYPES = [t[0] for t in TYPES] + ["complex_" + t[0] for t in TYPES]
AVERAGE = [1, 2, 3, 7, 64, 512]
CASCADE = [1, 2, 3]
PATTERNS = ["low", "full", "alt"]
LENGTH = {1: 32, 2: 32, 3: 32, 7: 48, 64: 160, 512: 560}     # samples per case (a prefix of the stored stream)
NMAX = max(LENGTH.values())

RING_DEQUE = r"""
#pragma once
#include <cstddef>
#include <deque>
namespace Pothos { namespace Util {
template <typename T> class RingDeque {
public:
    void clear() { _d.clear(); }
    void set_capacity(size_t n) { _cap = n; }
    bool full() const { return _d.size() >= _cap; }
    void push_back(const T &v) { _d.push_back(v); }
    void pop_front() { _d.pop_front(); }
    const T &front() const { return _d.front(); }
private:
    std::deque<T> _d;
    size_t _cap = 0;
};
}}
"""

DRIVER = r"""
// driver <scalar> <complex> <D> <C> <n> <in.bin> <out.bin>: DCRemoval::work's loop over one buffer
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "MovingAverage.hpp"

template <typename Type, typename AccType>
static int run(size_t D, size_t C, size_t n, const char *fin, const char *fout)
{
    std::vector<Type> in(n), out(n);
    FILE *f = std::fopen(fin, "rb");
    if (!f || std::fread(in.data(), sizeof(Type), n, f) != n) return 2;
    std::fclose(f);
    std::vector<MovingAverage<Type, AccType>> filters(C);
    for (auto &m : filters) m.resize(D);
    for (size_t i = 0; i < n; i++) {
        auto y = in[i];
        for (auto &m : filters) y = m(y);
        out[i] = filters[0].front() - y;
    }
    f = std::fopen(fout, "wb");
    if (!f || std::fwrite(out.data(), sizeof(Type), n, f) != n) return 3;
    std::fclose(f);
    return 0;
}
template <typename T, typename A>
static int pick(int cplx, size_t D, size_t C, size_t n, const char *fin, const char *fout)
{
    return cplx ? run<std::complex<T>, std::complex<A>>(D, C, n, fin, fout) : run<T, A>(D, C, n, fin, fout);
}
int main(int argc, char **argv)
{
    if (argc != 8) return 1;
    const int s = std::atoi(argv[1]), c = std::atoi(argv[2]);
    const size_t D = std::strtoull(argv[3], 0, 10), C = std::strtoull(argv[4], 0, 10), n = std::strtoull(argv[5], 0, 10);
    switch (s) {
    case 0: return pick<double, double>(c, D, C, n, argv[6], argv[7]);
    case 1: return pick<float, float>(c, D, C, n, argv[6], argv[7]);
    case 2: return pick<int64_t, int64_t>(c, D, C, n, argv[6], argv[7]);
    case 3: return pick<int32_t, int64_t>(c, D, C, n, argv[6], argv[7]);
    case 4: return pick<int16_t, int32_t>(c, D, C, n, argv[6], argv[7]);
    case 5: return pick<int8_t, int16_t>(c, D, C, n, argv[6], argv[7]);
    }
    return 1;
}
"""


def type_info(dtype):
    cplx = dtype.startswith("complex_")
    name = dtype[8:] if cplx else dtype
    for t in TYPES:
        if t[0] == name:
            return t[1], cplx, np.dtype(t[2]), t[3]
    raise ValueError(dtype)


def refused(dtype, D):
    """the divisor narrowed to the accumulator type is zero (the reference's integer division by zero)"""
    _, cplx, np_t, abits = type_info(dtype)
    if abits == 0:
        return False
    m = 1 << abits
    d = D % m
    return (d * d % m if cplx else d) == 0


def make_input(dtype, pattern, n, seed):
    _, cplx, np_t, _ = type_info(dtype)
    rng = np.random.default_rng(seed)
    shape = (n, 2) if cplx else (n,)
    if np_t.kind == "f":
        amp = 1e-3 if pattern == "low" else 1.0
        if pattern == "alt":
            x = np.where(np.arange(n) % 2 == 0, amp, -amp)
            x = np.repeat(x[:, None], 2, axis=1) if cplx else x
        else:
            x = rng.uniform(-amp, amp, shape)
        return x.astype(np_t)
    info = np.iinfo(np_t)
    if pattern == "alt":
        x = np.where(np.arange(n) % 2 == 0, info.max, info.min).astype(np_t)
        return np.repeat(x[:, None], 2, axis=1) if cplx else x
    if pattern == "low":
        return rng.integers(-3, 4, shape).astype(np_t)
    return rng.integers(info.min, info.max, shape, endpoint=True, dtype=np_t)


def build_driver(workdir):
    """compile DRIVER against the reference's MovingAverage.hpp into workdir; returns the executable's path"""
    os.makedirs(os.path.join(workdir, "Pothos", "Util"), exist_ok=True)
    with open(os.path.join(workdir, "Pothos", "Util", "RingDeque.hpp"), "w") as f:
        f.write(RING_DEQUE)
    src = os.path.join(workdir, "dcr_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(workdir, "dcr_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + workdir, "-I" + os.path.join(REF, "filter"), src, "-o", exe])
    return exe


def run_driver(exe, workdir, dtype, D, C, x):
    scalar, cplx, np_t, _ = type_info(dtype)
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    np.ascontiguousarray(x).tofile(fin)
    n = x.shape[0]
    subprocess.check_call([exe, str(scalar), str(int(cplx)), str(D), str(C), str(n), fin, fout])
    return np.fromfile(fout, dtype=np_t).reshape(x.shape)


def case_key(dtype, pattern, D, C):
    return "out/%s/%s/%d/%d" % (dtype, pattern, D, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "dcremoval.npz"))
    a = ap.parse_args()
    if not os.path.isdir(REF):
        sys.exit("the reference tree is not here: nothing to record")
    arrays = {}
    refused_cases = []
    with tempfile.TemporaryDirectory() as wd:
        exe = build_driver(wd)
        for ti, dtype in enumerate(DTYPES):
            for pi, pattern in enumerate(PATTERNS):
                x = make_input(dtype, pattern, NMAX, 1000 + 10 * ti + pi)
                arrays["in/%s/%s" % (dtype, pattern)] = x
                for D in AVERAGE:
                    for C in CASCADE:
                        if refused(dtype, D):
                            refused_cases.append("%s/%d/%d" % (dtype, D, C))
                            continue
                        arrays[case_key(dtype, pattern, D, C)] = run_driver(exe, wd, dtype, D, C, x[:LENGTH[D]])
    arrays["refused"] = np.array(sorted(set(refused_cases)))
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d cases, %d refused configurations, %d bytes" % (a.out, sum(k.startswith("out/") for k in arrays),
                                                                        len(set(refused_cases)), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
