"""Writes tests/golden/threshold.npz: /comms/threshold's labels as the reference's loop posts them.

A small driver of this project's own (DRIVER below) is compiled with the oracle's flags (g++ -O3 -ffp-contract=off, no -march) and
replays the loop of Threshold::work (utility/Threshold.cpp:130-144) over a stream cut into several calls: per call every element is
consumed, the active state is carried, and a label's index counts from the call's first element.  The driver records every state
change, whatever the IDs are (an empty ID drops the label, not the change).  Nothing compiled is kept.

Cases: the 6 element types x level pairs (activation above, equal to -- the default 0, 0 -- and below the deactivation level: the
last makes the toggle band) x inputs: seeded noise spanning both levels, a slow ramp up and down (few crossings), values inside
the toggle band only, the extremes (MIN / MAX / 0 / -1 mixes, for floats also NaN, +-inf and -0.0).  Every stream is fed in the
calls CUTS.  Recorded per case: the input, the two levels as elements of the type, and for every state change its index in the
whole stream, its kind (1 activation, 0 deactivation) and the state behind the stream.

    python tests/golden/make_threshold_golden.py [--out tests/golden/threshold.npz]
"""
import argparse
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

TYPES = [("float64", 0, np.float64), ("float32", 1, np.float32), ("int64", 2, np.int64), ("int32", 3, np.int32),
         ("int16", 4, np.int16), ("int8", 5, np.int8)]
LEVELS = {"above": (40, -25), "equal": (0, 0), "below": (-25, 40)}      # (activation, deactivation)
PATTERNS = ["noise", "ramp", "band", "extremes"]
N = 300
CUTS = [1, 37, 100, 11, 151]         # elements handed to each call; sums to N

DRIVER = r"""
// driver <scalar> <n> <ncuts> <cut...> <levels.bin> <in.bin> <out.bin>
// levels.bin: activation, deactivation as elements of the type.  out.bin: uint64 records -- the number of state changes, then per
// change (index in the whole stream, kind), then the state behind the stream.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <typename T>
static int run(size_t n, const std::vector<size_t> &cuts, const char *flv, const char *fin, const char *fout)
{
    T lv[2];
    std::vector<T> in(n);
    FILE *f = std::fopen(flv, "rb");
    if (!f || std::fread(lv, sizeof(T), 2, f) != 2) return 2;
    std::fclose(f);
    f = std::fopen(fin, "rb");
    if (!f || std::fread(in.data(), sizeof(T), n, f) != n) return 2;
    std::fclose(f);
    const T act = lv[0], deact = lv[1];
    bool active = false;
    std::vector<uint64_t> rec(1, 0);
    size_t pos = 0;
    for (size_t c : cuts) {
        const T *x = in.data() + pos;
        for (size_t i = 0; i < c; i++) {
            if (!active && x[i] > act) {
                active = true;
                rec.push_back(pos + i); rec.push_back(1);
            } else if (active && x[i] < deact) {
                active = false;
                rec.push_back(pos + i); rec.push_back(0);
            }
        }
        pos += c;
    }
    rec[0] = (rec.size() - 1) / 2;
    rec.push_back(active ? 1 : 0);
    f = std::fopen(fout, "wb");
    if (!f || std::fwrite(rec.data(), sizeof(uint64_t), rec.size(), f) != rec.size()) return 3;
    std::fclose(f);
    return 0;
}
int main(int argc, char **argv)
{
    if (argc < 7) return 1;
    const int s = std::atoi(argv[1]);
    const size_t n = std::strtoull(argv[2], 0, 10), nc = std::strtoull(argv[3], 0, 10);
    if ((size_t)argc != 7 + nc) return 1;
    std::vector<size_t> cuts;
    size_t sum = 0;
    for (size_t i = 0; i < nc; i++) { cuts.push_back(std::strtoull(argv[4 + i], 0, 10)); sum += cuts.back(); }
    if (sum != n) return 1;
    const char *flv = argv[4 + nc], *fi = argv[5 + nc], *fo = argv[6 + nc];
    switch (s) {
    case 0: return run<double>(n, cuts, flv, fi, fo);
    case 1: return run<float>(n, cuts, flv, fi, fo);
    case 2: return run<int64_t>(n, cuts, flv, fi, fo);
    case 3: return run<int32_t>(n, cuts, flv, fi, fo);
    case 4: return run<int16_t>(n, cuts, flv, fi, fo);
    case 5: return run<int8_t>(n, cuts, flv, fi, fo);
    }
    return 1;
}
"""


def make_input(np_t, pattern, levels, n, seed):
    rng = np.random.default_rng(seed)
    np_t = np.dtype(np_t)
    lo, hi = min(levels), max(levels)
    if pattern == "noise":
        x = rng.uniform(lo - 60, hi + 60, n)
    elif pattern == "ramp":
        x = 100.0 * np.sin(np.arange(n) * (2 * np.pi / 97.0)) + rng.uniform(-3, 3, n)
    elif pattern == "band":                     # strictly between the levels where there is room, on them where there is none
        x = rng.uniform(lo + 1, hi - 1, n) if hi - lo > 2 else np.full(n, float(lo))
    else:
        if np_t.kind == "f":
            fi = np.finfo(np_t)
            vals = np.array([fi.max, -fi.max, fi.tiny, -fi.tiny, 0.0, -0.0, 1.0, -1.0, np.nan, np.inf, -np.inf, 40.0, -25.0], dtype=np_t)
        else:
            info = np.iinfo(np_t)
            vals = np.array([info.min, info.max, 0, -1, 1, info.min + 1, info.max - 1, 40, -25, 41, -26], dtype=np_t)
        return rng.choice(vals, n)
    return (x if np_t.kind == "f" else np.rint(x)).astype(np_t)


def build_driver(workdir):
    src = os.path.join(workdir, "thr_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(workdir, "thr_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", src, "-o", exe])
    return exe


def run_driver(exe, workdir, scalar, lv, x, cuts):
    flv, fin, fout = (os.path.join(workdir, n) for n in ("levels.bin", "in.bin", "out.bin"))
    np.ascontiguousarray(lv).tofile(flv)
    np.ascontiguousarray(x).tofile(fin)
    subprocess.check_call([exe, str(scalar), str(x.size), str(len(cuts))] + [str(c) for c in cuts] + [flv, fin, fout])
    rec = np.fromfile(fout, dtype=np.uint64)
    k = int(rec[0])
    assert rec.size == 2 * k + 2
    return rec[1:1 + 2 * k:2].copy(), rec[2:2 + 2 * k:2].astype(np.uint8), int(rec[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "threshold.npz"))
    a = ap.parse_args()
    assert sum(CUTS) == N
    arrays = {"cuts": np.array(CUTS)}
    with tempfile.TemporaryDirectory() as wd:
        exe = build_driver(wd)
        for ti, (name, scalar, np_t) in enumerate(TYPES):
            for li, (lk, levels) in enumerate(LEVELS.items()):
                lv = np.array(levels, dtype=np_t)
                for pi, pattern in enumerate(PATTERNS):
                    x = make_input(np_t, pattern, levels, N, 3000 + 100 * ti + 10 * li + pi)
                    key = "%s/%s/%s" % (name, lk, pattern)
                    idx, kind, final = run_driver(exe, wd, scalar, lv, x, CUTS)
                    arrays["in/" + key] = x
                    arrays["levels/" + key] = lv
                    arrays["idx/" + key] = idx
                    arrays["kind/" + key] = kind
                    arrays["final/" + key] = np.array(final, np.uint8)
            # a NaN level never compares true (floats only)
            if np.dtype(np_t).kind == "f":
                for lk, lv in (("nan_act", np.array([np.nan, 0], np_t)), ("nan_deact", np.array([0, np.nan], np_t))):
                    x = make_input(np_t, "noise", (-25, 40), N, 3900 + ti)
                    key = "%s/%s/noise" % (name, lk)
                    idx, kind, final = run_driver(exe, wd, scalar, lv, x, CUTS)
                    arrays.update({"in/" + key: x, "levels/" + key: lv, "idx/" + key: idx, "kind/" + key: kind,
                                   "final/" + key: np.array(final, np.uint8)})
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d cases, %d bytes" % (a.out, sum(k.startswith("idx/") for k in arrays), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
