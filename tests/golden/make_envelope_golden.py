"""Writes tests/golden/envelope.npz: /comms/envelope_detector's outputs as the reference computes them.

Run where the reference tree exists.  A small driver of this project's own (DRIVER below) is compiled with the oracle's flags
(g++ -O3 -ffp-contract=off, no -march) against the reference's functions/FxptHelpers.hpp (getAbs) and replays the loop of
EnvelopeDetector::work over a stream cut into several calls: per call, N = elements - lookahead outputs from in[i + lookahead],
N consumed, the envelope carried.  Nothing compiled is kept.

Cases: the 12 element types x (attack, release) in {(10, 10), (1, 50), (0, 10), (1000, 3), never set (all gains 0)} x lookahead
in {0, 10} x inputs: seeded noise at low and at full scale, the extremes (MIN / MAX / 0 / -1 mixes), equal-magnitude complex pairs
(integers) and a burst followed by zeros (the envelope decays through the subnormals); for floats also NaN, +-inf and -0.0 spread
through the stream.  Every stream is fed in the calls CUTS.

    python tests/golden/make_envelope_golden.py [--out tests/golden/envelope.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("PCX_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

TYPES = [("float64", 0, np.float64), ("float32", 1, np.float32), ("int64", 2, np.int64), ("int32", 3, np.int32),
         ("int16", 4, np.int16), ("int8", 5, np.int8)]
DTYPES = [t[0] for t in TYPES] + ["complex_" + t[0] for t in TYPES]
TIMES = {"10_10": (10.0, 10.0), "1_50": (1.0, 50.0), "0_10": (0.0, 10.0), "1000_3": (1000.0, 3.0), "unset": None}
LOOKAHEAD = [0, 10]
N = 400
CUTS = [1, 37, 100, 11, 251]         # input elements handed to each call; sums to N


def patterns(dtype):
    names = ["low", "full", "extremes", "burst"]
    if dtype.startswith("complex_") and "int" in dtype:
        names.append("pairs")
    if "float" in dtype:
        names.append("special")
    return names


DRIVER = r"""
// driver <scalar> <complex> <mode> <attack> <release> <lookahead> <n> <ncuts> <cut...> <in.bin> <out.bin>
// mode 1: setAttack / setRelease called; 0: never called (all gains 0).  Replays EnvelopeDetector::work's loop call by call.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "FxptHelpers.hpp"

template <typename In>
static int run(int mode, float attack, float release, size_t L, size_t n, const std::vector<size_t> &cuts, const char *fin,
               const char *fout)
{
    std::vector<In> in(n);
    FILE *f = std::fopen(fin, "rb");
    if (!f || std::fread(in.data(), sizeof(In), n, f) != n) return 2;
    std::fclose(f);
    float env = 0, gA = 0, gR = 0, oA = 0, oR = 0;
    if (mode) {
        gA = std::exp(-1 / attack); oA = 1 - gA;
        gR = std::exp(-1 / release); oR = 1 - gR;
    }
    std::vector<float> out;
    size_t pos = 0, avail = 0;           // first unconsumed element, elements in the buffer
    for (size_t c : cuts) {
        avail += c;
        if (avail <= L) continue;
        const size_t N = avail - L;
        for (size_t i = 0; i < N; i++) {
            const float xn = getAbs<float>(in[pos + i + L]);
            if (xn > env) env = gA * env + oA * xn;
            else env = gR * env + oR * xn;
            out.push_back(env);
        }
        pos += N;
        avail -= N;
    }
    f = std::fopen(fout, "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 3;
    std::fclose(f);
    return 0;
}
template <typename T>
static int pick(int cplx, int mode, float a, float r, size_t L, size_t n, const std::vector<size_t> &cuts, const char *fi, const char *fo)
{
    return cplx ? run<std::complex<T>>(mode, a, r, L, n, cuts, fi, fo) : run<T>(mode, a, r, L, n, cuts, fi, fo);
}
int main(int argc, char **argv)
{
    if (argc < 11) return 1;
    const int s = std::atoi(argv[1]), c = std::atoi(argv[2]), mode = std::atoi(argv[3]);
    const float a = std::strtof(argv[4], 0), r = std::strtof(argv[5], 0);
    const size_t L = std::strtoull(argv[6], 0, 10), n = std::strtoull(argv[7], 0, 10), nc = std::strtoull(argv[8], 0, 10);
    if ((size_t)argc != 11 + nc) return 1;
    std::vector<size_t> cuts;
    for (size_t i = 0; i < nc; i++) cuts.push_back(std::strtoull(argv[9 + i], 0, 10));
    const char *fi = argv[9 + nc], *fo = argv[10 + nc];
    switch (s) {
    case 0: return pick<double>(c, mode, a, r, L, n, cuts, fi, fo);
    case 1: return pick<float>(c, mode, a, r, L, n, cuts, fi, fo);
    case 2: return pick<int64_t>(c, mode, a, r, L, n, cuts, fi, fo);
    case 3: return pick<int32_t>(c, mode, a, r, L, n, cuts, fi, fo);
    case 4: return pick<int16_t>(c, mode, a, r, L, n, cuts, fi, fo);
    case 5: return pick<int8_t>(c, mode, a, r, L, n, cuts, fi, fo);
    }
    return 1;
}
"""


def type_info(dtype):
    cplx = dtype.startswith("complex_")
    name = dtype[8:] if cplx else dtype
    for t in TYPES:
        if t[0] == name:
            return t[1], cplx, np.dtype(t[2])
    raise ValueError(dtype)


def make_input(dtype, pattern, n, seed):
    _, cplx, np_t = type_info(dtype)
    rng = np.random.default_rng(seed)
    shape = (n, 2) if cplx else (n,)
    if np_t.kind == "f":
        if pattern in ("low", "full"):
            amp = 1e-3 if pattern == "low" else 1e3
            x = rng.uniform(-amp, amp, shape)
        elif pattern == "extremes":
            fi = np.finfo(np_t)
            x = rng.choice(np.array([fi.max, -fi.max, fi.tiny, -fi.tiny, 0.0, 1.0, -1.0], dtype=np_t), shape)
        elif pattern == "burst":
            x = np.zeros(shape)
            x[:60] = rng.uniform(-1, 1, x[:60].shape)
        else:   # special: noise with NaN, +-inf, -0.0 dropped in
            x = rng.uniform(-1, 1, shape)
            flat = x.reshape(-1)
            for v, at in ((np.nan, 300), (np.inf, 100), (-np.inf, 150), (-0.0, 50), (-0.0, 51), (np.inf, 380)):
                flat[at] = v
        return x.astype(np_t)
    info = np.iinfo(np_t)
    if pattern == "low":
        return rng.integers(-3, 4, shape).astype(np_t)
    if pattern == "full":
        return rng.integers(info.min, info.max, shape, endpoint=True, dtype=np_t)
    if pattern == "extremes":
        vals = [info.min, info.max, 0, -1, 1, info.min + 1]
        if cplx:
            # (MIN, 0) is outside what the reference can compute for complex_int32 / complex_int64: abs(MIN) wraps to MIN, the
            # compiled header then divides by zero (SIGFPE).  Zeros stay out of the complex extremes.
            vals.remove(0)
        return rng.choice(np.array(vals, dtype=np_t), shape)
    if pattern == "burst":
        x = np.zeros(shape, np_t)
        x[:60] = rng.integers(info.min, info.max, x[:60].shape, endpoint=True, dtype=np_t)
        return x
    # pairs: equal magnitudes in both components (s * sqrt(2) truncated), the whole range
    v = rng.integers(info.min, info.max, n, endpoint=True, dtype=np_t)
    sgn = rng.choice(np.array([1, -1], dtype=np.int64), n)
    w = (v.astype(np.int64) * sgn)
    w = np.where(w > info.max, info.min, w).astype(np_t)
    return np.stack([v, w], axis=1)


def build_driver(workdir):
    src = os.path.join(workdir, "env_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(workdir, "env_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(REF, "functions"),
                           src, "-o", exe])
    return exe


def run_driver(exe, workdir, dtype, times, L, x, cuts):
    scalar, cplx, _ = type_info(dtype)
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    np.ascontiguousarray(x).tofile(fin)
    a, r = times if times is not None else (0.0, 0.0)
    args = [exe, str(scalar), str(int(cplx)), "0" if times is None else "1", repr(float(a)), repr(float(r)), str(L), str(x.shape[0]),
            str(len(cuts))] + [str(c) for c in cuts] + [fin, fout]
    subprocess.check_call(args)
    return np.fromfile(fout, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "envelope.npz"))
    a = ap.parse_args()
    if not os.path.isdir(REF):
        sys.exit("the reference tree is not here: nothing to record")
    assert sum(CUTS) == N
    arrays = {"cuts": np.array(CUTS)}
    with tempfile.TemporaryDirectory() as wd:
        exe = build_driver(wd)
        for ti, dtype in enumerate(DTYPES):
            for pi, pattern in enumerate(patterns(dtype)):
                x = make_input(dtype, pattern, N, 2000 + 10 * ti + pi)
                arrays["in/%s/%s" % (dtype, pattern)] = x
                for tk, times in TIMES.items():
                    for L in LOOKAHEAD:
                        arrays["out/%s/%s/%s/%d" % (dtype, pattern, tk, L)] = run_driver(exe, wd, dtype, times, L, x, CUTS)
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d cases, %d bytes" % (a.out, sum(k.startswith("out/") for k in arrays), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
