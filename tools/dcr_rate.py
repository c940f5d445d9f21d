"""The rate of /comms/dc_removal on the device, both paths, at 64 Mi samples per call: one JSON line.

  fused   complex_float32 at the defaults (average 512, cascade 2): one launch; 16 bytes of HBM traffic per sample at the least
          (8 in, 8 out), plus the halo the workgroups re-read
  staged  complex_int16 at the defaults: per stage reduce, scan, apply (the increment narrows to int16, so nothing telescopes)

Device-resident input and output (process_dev), hip events around `--reps` back-to-back calls after `--warmup` calls, median of
`--trials` windows.  python tools/dcr_rate.py [--n 67108864] [--reps 20] [--warmup 5] [--trials 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12     # bytes/s, MI355X_MICROARCH.md


def time_path(dev, torch, dtype, n, reps, warmup, trials):
    scalar = {"complex_float32": torch.float32, "complex_int16": torch.int16}[dtype]
    if scalar == torch.float32:
        x = torch.empty((n, 2), dtype=torch.float32, device="cuda:0")
        dev.fill_uniform_f32_dev(x, seed=1)
    else:
        x = torch.randint(-32768, 32767, (n, 2), dtype=torch.int16, device="cuda:0")
    y = torch.empty_like(x)
    h = dev.DCRemoval(dtype)
    s = torch.cuda.current_stream()
    for _ in range(warmup):
        h.process_dev(x, y, n, stream=s)
    torch.cuda.synchronize()
    times = []
    for _ in range(trials):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            h.process_dev(x, y, n, stream=s)
        e1.record(s)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / reps)
    times.sort()
    t = times[len(times) // 2]
    bytes_min = 2 * n * x.element_size() * 2          # one read and one write of every sample
    return {"dtype": dtype, "samples": n, "call_ms": round(t * 1e3, 4), "gsamples_per_s": round(n / t / 1e9, 2),
            "hbm_share_min_bytes": round(bytes_min / t / HBM_PEAK, 3), "spread": round(times[-1] / times[0] - 1, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trials", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("dcr_rate: no GPU")
    from pothoscomms_amd import device as dev
    out = {"metric": "dc_removal_rate",
           "fused": time_path(dev, torch, "complex_float32", a.n, a.reps, a.warmup, a.trials),
           "staged": time_path(dev, torch, "complex_int16", a.n, a.reps, a.warmup, a.trials)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
