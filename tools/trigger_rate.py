"""The rate of /comms/wave_trigger's level search on the device at 64 Mi elements per call: one JSON line.

float32, complex_float32, complex_int16, int8 and float64 streams of uniform noise below the level, with the only crossing on the last
pair (the whole stream is read) and, for float32, with the crossing a quarter of the way in (the workgroups behind it leave early).
Device-resident buffers, search_dev: a memset of the word the workgroups meet in, the search, and the launch that writes the 24 bytes.
Hip events around `--reps` back-to-back calls after `--warmup` calls, the windows of the variants and of a device-to-device copy of the
same input bytes alternating, median of `--trials` windows with their spread (max / min - 1).  Each entry gives TB/s of input READ (the
copy reads and writes that many bytes: its rate counts both), the ratio of the copy's time to the call's, and whether the input fits
the 256 MiB of MALL (then the repetitions of a window find it there: not a cold rate) or streams from HBM.
    python tools/trigger_rate.py [--n 67108864] [--reps 50] [--warmup 3] [--trials 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_rate import MALL_BYTES, windows_of  # noqa: E402

TYPES = ("float32", "complex_float32", "complex_int16", "int8", "float64")


def time_case(dev, torch, dtype, n, reps, warmup, trials):
    cplx = dtype.startswith("complex_")
    scalar = dtype[8:] if cplx else dtype
    tdt = {"float32": torch.float32, "float64": torch.float64, "int16": torch.int16, "int8": torch.int8}[scalar]
    shape = (n, 2) if cplx else (n,)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    x = torch.rand(shape, device="cuda:0", generator=g) * 40 - 20          # |x| < 29: below the level throughout
    x = (x if tdt.is_floating_point else x.round()).to(tdt)
    x[n - 1] = 100
    y = torch.empty_like(x)
    hit = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream()
    h = dev.Trigger(dtype, 50.0, "POS")
    variants = [("hit_on_the_last_pair", lambda: h.search_dev(x, n, 0, hit, stream=s))]
    expect = [n - 2]
    if dtype == "float32":
        xq = x.clone()
        xq[n // 4] = 100
        variants.append(("hit_a_quarter_in", lambda: h.search_dev(xq, n, 0, hit, stream=s)))
        expect.append(n // 4 - 1)
    for (name, f), want in zip(variants, expect):                          # the answer first
        f()
        torch.cuda.synchronize()
        got = hit.cpu().tolist()
        assert (got[0], got[2]) == (want, 1), (dtype, name, got, want)
    variants.append(("d2d_copy", lambda: y.copy_(x)))
    res = windows_of(torch, [f for _, f in variants], reps, warmup, trials)
    nbytes = x.numel() * x.element_size()
    tcopy = res[-1][0]
    out = {"dtype": dtype, "elements": n, "input_bytes": nbytes, "d2d_copy_ms": round(tcopy * 1e3, 4),
           "d2d_copy_tb_per_s": round(2 * nbytes / tcopy / 1e12, 3), "d2d_copy_spread": round(res[-1][1], 4),
           "input": "fits the MALL" if nbytes <= MALL_BYTES else "streams from HBM", "tile": h.geometry()}
    for (name, _), (t, sp) in zip(variants[:-1], res[:-1]):
        out[name] = {"call_ms": round(t * 1e3, 4), "read_tb_per_s": round(nbytes / t / 1e12, 3), "spread": round(sp, 4),
                     "copy_time_over_call_time": round(tcopy / t, 3)}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--types", default=",".join(TYPES))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("trigger_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = [time_case(dev, torch, dtype, a.n, a.reps, a.warmup, a.trials) for dtype in a.types.split(",")]
    print(json.dumps({"metric": "trigger_rate", "elements": a.n, "reps": a.reps, "warmup": a.warmup, "trials": a.trials, "cases": cases}))


if __name__ == "__main__":
    main()
