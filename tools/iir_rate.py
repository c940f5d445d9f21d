"""The rate of /comms/iir_filter on the device at 64 Mi samples per call: one JSON line.

complex_float32, float32, complex_int16 and complex_float64 at the reference's default taps (order 2), a 4th-order Butterworth at 0.1
of the sample rate and an 8th-order one at 0.05 (both SCAN), device-resident input and output (process_dev), hip events around
`--reps` back-to-back calls after `--warmup` calls, median of `--trials` windows.  Each entry: Gsamples/s and the share of the HBM roof
at the bytes of two reads of the input and one write of the output per sample at 8 TB/s (complex_float32: 24 B, 333 Gsamples/s).
    python tools/iir_rate.py [--n 67108864] [--reps 10] [--warmup 3] [--trials 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12     # bytes/s, MI355X_MICROARCH.md


def time_case(dev, torch, dtype, fname, taps, n, reps, warmup, trials):
    cplx = dtype.startswith("complex")
    shape = (n, 2) if cplx else (n,)
    if dtype == "complex_int16":
        x = torch.randint(-32768, 32767, shape, dtype=torch.int16, device="cuda:0")
    else:
        x = torch.empty(shape, dtype=torch.float32, device="cuda:0")
        dev.fill_uniform_f32_dev(x, seed=1)
        if dtype == "complex_float64":
            x = x.to(torch.float64)
    y = torch.empty_like(x)
    h = dev.IIRFilter(dtype, taps)
    plan, bound = h.plan()
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
    elem = x.element_size() * (2 if cplx else 1)
    return {"dtype": dtype, "taps": fname, "plan": "SCAN" if plan == 0 else "SERIAL", "bound": bound, "samples": n,
            "call_ms": round(t * 1e3, 4), "gsamples_per_s": round(n / t / 1e9, 2), "hbm_roof_share": round(n * 3 * elem / t / HBM_PEAK, 3),
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
        sys.exit("iir_rate: no GPU")
    import iir_model as M
    from pothoscomms_amd import device as dev
    filters = {"default": M.DEFAULT_TAPS, "butter4_0.1": M.taps_of(M.butter(4, 0.2)), "butter8_0.05": M.taps_of(M.butter(8, 0.1))}
    cases = [time_case(dev, torch, dtype, fname, taps, a.n, a.reps, a.warmup, a.trials)
             for dtype in ("complex_float32", "float32", "complex_int16", "complex_float64") for fname, taps in filters.items()]
    print(json.dumps({"metric": "iir_filter_rate", "cases": cases}))


if __name__ == "__main__":
    main()
