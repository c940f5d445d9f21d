"""The rate of /comms/threshold on the device at 64 Mi elements per call: one JSON line.

int8, float32 and float64 streams, the levels of the toggle band (activation below deactivation), on two inputs: uniform noise
spanning both levels, and the dense stream whose every element is a transition.  Device-resident buffers, process_dev with `out`
separate, `out == in` and `out = None`, and with `out` separate but idx_cap 0 (classify and offsets alone: what the select step
costs is the difference).  Hip events around `--reps` back-to-back calls after `--warmup` calls, the windows of the variants and of
a device-to-device copy of the same tensors alternating, median of `--trials` windows with their spread (max / min - 1).  Each
entry gives TB/s of input plus output (the indices are counted apart), the ratio of the copy's time to the call's, and whether
input plus output (what the copy and the variant without indices touch), and these with the indices, fit the 256 MiB of MALL
(then the repetitions of a window find them there: not a cold rate) or stream from HBM.
    python tools/threshold_rate.py [--n 67108864] [--reps 100] [--warmup 3] [--trials 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MALL_BYTES = 256 << 20                  # MI355X_MICROARCH.md
LEVELS = (-25, 40)                      # activation, deactivation: everything between them toggles


def windows_of(torch, fns, reps, warmup, trials):
    """median seconds per call and spread of each function, their timed windows alternating"""
    s = torch.cuda.current_stream()
    for f in fns:
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(trials):
        for k, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                f()
            e1.record(s)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / 1e3 / reps)
    out = []
    for t in times:
        t.sort()
        out.append((t[len(t) // 2], t[-1] / t[0] - 1))
    return out


def time_case(dev, torch, dtype, kind, n, reps, warmup, trials):
    tdt = {"int8": torch.int8, "float32": torch.float32, "float64": torch.float64}[dtype]
    if kind == "noise":
        g = torch.Generator(device="cuda:0")
        g.manual_seed(7)
        x = (torch.rand(n, device="cuda:0", generator=g) * 185 - 85).round().to(tdt)        # -85 ... 100
    else:
        x = (torch.arange(n, device="cuda:0") % 2).to(tdt)                                  # 0, 1, 0, 1 ...: inside the band
    y = torch.empty_like(x)
    idx = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    h = dev.Threshold(dtype, *LEVELS)
    s = torch.cuda.current_stream()
    variants = [("out_separate", lambda: h.process_dev(x, n, idx, n, counts, out=y, stream=s)),
                ("out_in_place", lambda: h.process_dev(x, n, idx, n, counts, out=x, stream=s)),
                ("out_none", lambda: h.process_dev(x, n, idx, n, counts, stream=s)),
                ("out_separate_no_indices", lambda: h.process_dev(x, n, idx, 0, counts, out=y, stream=s)),
                ("d2d_copy", lambda: y.copy_(x))]
    res = windows_of(torch, [f for _, f in variants], reps, warmup, trials)
    h.process_dev(x, n, idx, n, counts, out=y, stream=s)
    torch.cuda.synchronize()
    _, ntrans, _ = counts.tolist()
    es = x.element_size()
    tcopy = res[-1][0]
    out = {"dtype": dtype, "input": kind, "elements": n, "transitions": ntrans, "index_bytes": 8 * ntrans,
           "d2d_copy_ms": round(tcopy * 1e3, 4), "d2d_copy_tb_per_s": round(2 * n * es / tcopy / 1e12, 3), "d2d_copy_spread": round(res[-1][1], 4),
           "stream_tensors": "fit the MALL" if 2 * n * es <= MALL_BYTES else "stream from HBM",
           "with_indices": "fit the MALL" if 2 * n * es + 8 * ntrans <= MALL_BYTES else "stream from HBM"}
    for (name, _), (t, sp) in zip(variants[:-1], res[:-1]):
        moved = n * es * (1 if name == "out_none" else 2)
        out[name] = {"call_ms": round(t * 1e3, 4), "tb_per_s": round(moved / t / 1e12, 3), "spread": round(sp, 4), "copy_time_over_call_time": round(tcopy / t, 3)}
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("threshold_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = [time_case(dev, torch, dtype, kind, a.n, a.reps, a.warmup, a.trials) for dtype in ("int8", "float32", "float64") for kind in ("noise", "dense")]
    print(json.dumps({"metric": "threshold_rate", "elements": a.n, "reps": a.reps, "warmup": a.warmup, "trials": a.trials, "cases": cases}))


if __name__ == "__main__":
    main()
