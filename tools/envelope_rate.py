"""The rate of /comms/envelope_detector on the device at 64 Mi samples per call: one JSON line.

complex_float32, float32 and complex_int16 at attack / release 10/10, 100/100 and 1000/1000, lookahead 10, device-resident input
and output (process_dev), hip events around `--reps` back-to-back calls after `--warmup` calls, median of `--trials` windows.
Each entry: Gsamples/s, the share of the HBM roof (bytes of one read of the input and one write of the output per sample at
8 TB/s; complex_float32: 12 B, 667 Gsamples/s) and the path counts of the last call (pcx_envelope_get_stats).
    python tools/envelope_rate.py [--n 67108864] [--reps 10] [--warmup 3] [--trials 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12     # bytes/s, MI355X_MICROARCH.md
L = 10


def time_case(dev, torch, dtype, tc, n, reps, warmup, trials):
    if dtype == "complex_int16":
        x = torch.randint(-32768, 32767, (n + L, 2), dtype=torch.int16, device="cuda:0")
    else:
        x = torch.empty((n + L, 2) if dtype.startswith("complex") else (n + L,), dtype=torch.float32, device="cuda:0")
        dev.fill_uniform_f32_dev(x, seed=1)
    y = torch.empty(n, dtype=torch.float32, device="cuda:0")
    h = dev.EnvelopeDetector(dtype, attack=tc, release=tc, lookahead=L)
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
    bytes_per = x.element_size() * (2 if x.dim() == 2 else 1) + 4
    chunks, repaired, resolved = h.stats()
    return {"dtype": dtype, "attack_release": tc, "samples": n, "call_ms": round(t * 1e3, 4), "gsamples_per_s": round(n / t / 1e9, 2),
            "hbm_roof_share": round(n * bytes_per / t / HBM_PEAK, 3), "chunks": chunks, "repaired": repaired, "resolved": resolved,
            "spread": round(times[-1] / times[0] - 1, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("envelope_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = [time_case(dev, torch, dtype, tc, a.n, a.reps, a.warmup, a.trials)
             for dtype in ("complex_float32", "float32", "complex_int16") for tc in (10.0, 100.0, 1000.0)]
    print(json.dumps({"metric": "envelope_detector_rate", "cases": cases}))


if __name__ == "__main__":
    main()
