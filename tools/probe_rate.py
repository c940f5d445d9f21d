"""The rate of /comms/signal_probe on the device at 64 Mi elements per call: one JSON line.

complex_float32, float32, complex_int16, int8 and complex_float64 streams of uniform noise, RMS and MEAN, with windows of 1024
elements (the small-window path: 1 to 16 KiB per window, a wave owns each) and with the whole call as one window (the
large-window path: a partial per slice, then the join).  Device-resident buffers, windows_dev.  Hip events around `--reps`
back-to-back calls after `--warmup` calls, the windows of the variants and of a device-to-device copy of the same input bytes
alternating, median of `--trials` windows with their spread (max / min - 1).  Each entry gives TB/s of input READ (the copy reads
and writes that many bytes: its rate counts both), the ratio of the copy's time to the call's, and whether the input fits the
256 MiB of MALL (then the repetitions of a window find it there: not a cold rate) or streams from HBM.
    python tools/probe_rate.py [--n 67108864] [--reps 50] [--warmup 3] [--trials 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MALL_BYTES = 256 << 20                  # MI355X_MICROARCH.md
TYPES = ("complex_float32", "float32", "complex_int16", "int8", "complex_float64")


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


def time_case(dev, torch, dtype, n, reps, warmup, trials):
    cplx = dtype.startswith("complex_")
    scalar = dtype[8:] if cplx else dtype
    tdt = {"float32": torch.float32, "float64": torch.float64, "int16": torch.int16, "int8": torch.int8}[scalar]
    shape = (n, 2) if cplx else (n,)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    x = torch.rand(shape, device="cuda:0", generator=g) * 200 - 100
    x = (x if tdt.is_floating_point else x.round()).to(tdt)
    y = torch.empty_like(x)
    values = torch.zeros((-(-n // 1024), 2), dtype=torch.float64, device="cuda:0")
    s = torch.cuda.current_stream()
    variants, handles = [], []
    for mode in ("RMS", "MEAN"):
        for name, window in (("window_1024", 1024), ("window_whole_call", n)):
            h = dev.SignalProbe(dtype, mode, window)
            handles.append(h)
            variants.append(("%s_%s" % (mode.lower(), name), (lambda h=h: h.windows_dev(x, n, values, stream=s))))
    variants.append(("d2d_copy", lambda: y.copy_(x)))
    res = windows_of(torch, [f for _, f in variants], reps, warmup, trials)
    nbytes = x.numel() * x.element_size()
    tcopy = res[-1][0]
    out = {"dtype": dtype, "elements": n, "input_bytes": nbytes, "d2d_copy_ms": round(tcopy * 1e3, 4),
           "d2d_copy_tb_per_s": round(2 * nbytes / tcopy / 1e12, 3), "d2d_copy_spread": round(res[-1][1], 4),
           "input": "fits the MALL" if nbytes <= MALL_BYTES else "streams from HBM", "tile_slice_switch": handles[0].geometry()}
    for (name, _), (t, sp) in zip(variants[:-1], res[:-1]):
        out[name] = {"call_ms": round(t * 1e3, 4), "read_tb_per_s": round(nbytes / t / 1e12, 3), "spread": round(sp, 4),
                     "copy_time_over_call_time": round(tcopy / t, 3)}
    for h in handles:
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
        sys.exit("probe_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = [time_case(dev, torch, dtype, a.n, a.reps, a.warmup, a.trials) for dtype in a.types.split(",")]
    print(json.dumps({"metric": "probe_rate", "elements": a.n, "reps": a.reps, "warmup": a.warmup, "trials": a.trials, "cases": cases}))


if __name__ == "__main__":
    main()
