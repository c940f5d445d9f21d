"""The rates of /comms/waveform_source and /comms/noise_source on the device at 64 Mi elements per call: a table, then one JSON line.

Cases, for complex_float32, complex_int16, float32 and complex_float64 each:
  step410  4096 entries walked with step 410 (freq 0.1 of the rate): a period of 2048 elements, short enough for LDS at some types
  step26   262144 entries walked with step 26 (freq 1e-4 of the rate): a period of 131072 elements, read from global memory
  noise    the noise source's walk: 4096 entries, step 1, the index moved by a draw in front of every call
(the table says per case whether the product stages the period in LDS)
and the same cases twice more through the diagnostic library (child processes that load libpcx_hip_diag.so): "gather", its
per-element gather (PCX_SRC_GATHER; the product has no such kernel), and "period_no_lds", the period form with every period read from
global memory (PCX_SRC_NO_LDS), the A/B partner of the LDS staging.

A source only writes, so a case is reported as bytes written per second.  The yardstick is a device fill of the same bytes:
hipMemsetAsync on the same buffer, in the same process and on the same stream, each window right after the case's own (alternating).
Device-resident output (generate_dev), hip events around as many back-to-back calls as fill `--window` seconds, after `--warmup`
calls; the median of `--trials` windows with their spread (slowest over fastest - 1).  Per case: the time over the fill's, and the
share of the HBM peak of MI355X_MICROARCH.md (8 TB/s).  The buffers are rewritten call after call, so these are warm-cache rates.
    python tools/source_rate.py [--n 67108864] [--window 0.3] [--warmup 3] [--trials 5] [--out FILE] [--no-gather]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                          # bytes/s
TYPES = ["complex_float32", "complex_int16", "float32", "complex_float64"]
ES = {"complex_float32": 8, "complex_int16": 4, "float32": 4, "complex_float64": 16}


def windows(torch, s, call, base, window, warmup, trials):
    """medians and spreads of `trials` alternating windows of the case and of the yardstick: (t_case, spread_case, t_base, spread_base)"""
    def one(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3 / reps
    for _ in range(warmup):
        call()
        base()
    torch.cuda.synchronize()
    reps_c = max(2, int(window / max(one(call, 2), 1e-6)) + 1)
    reps_b = max(2, int(window / max(one(base, 2), 1e-6)) + 1)
    tc, tb = [], []
    for _ in range(trials):
        tc.append(one(call, reps_c))
        tb.append(one(base, reps_b))
    tc.sort()
    tb.sort()
    return tc[len(tc) // 2], tc[-1] / tc[0] - 1, tb[len(tb) // 2], tb[-1] / tb[0] - 1


def measure_all(a, kernel):
    import torch
    if not torch.cuda.is_available():
        sys.exit("source_rate: no GPU")
    from pothoscomms_amd import _lib, device as dev
    _lib.load()
    rt = _lib._hip_runtime or C.CDLL("libamdhip64.so")
    rt.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    rt.hipMemsetAsync.restype = C.c_int
    s = torch.cuda.current_stream()
    out = torch.empty(a.n * 16, dtype=torch.uint8, device="cuda:0")
    cases = []
    for dt in TYPES:
        nbytes = a.n * ES[dt]

        def fill():
            if rt.hipMemsetAsync(C.c_void_p(out.data_ptr()), 0x5A, nbytes, C.c_void_p(s.cuda_stream)) != 0:
                sys.exit("source_rate: hipMemsetAsync failed")

        sources = [("step410", dev.WaveformSource(dt, "SINE", freq=0.1, ampl=100.0 if "int" in dt else 1.0)),
                   ("step26", dev.WaveformSource(dt, "SINE", freq=1e-4, ampl=100.0 if "int" in dt else 1.0)),
                   ("noise", dev.NoiseSource(dt, "NORMAL", b=100.0 if "int" in dt else 1.0, seed=1))]
        for name, src in sources:
            _, period, staged = src.geometry()
            t, sp, tb, spb = windows(torch, s, lambda: src.generate(a.n, out=out.data_ptr(), stream=s), fill, a.window, a.warmup, a.trials)
            cases.append({"case": "%s/%s/%s" % (kernel, dt, name), "elements": a.n, "period": period, "staged_in_lds": bool(staged) and kernel == "period",
                          "call_ms": round(t * 1e3, 4), "bytes_written": nbytes, "bytes_per_s": round(nbytes / t, 1), "spread": round(sp, 4),
                          "share_of_hbm_peak": round(nbytes / HBM_PEAK / t, 3), "fill_same_bytes_ms": round(tb * 1e3, 4),
                          "fill_bytes_per_s": round(nbytes / tb, 1), "fill_spread": round(spb, 4), "time_over_fill": round(t / tb, 3)})
            src.close()
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20, help="elements per call")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    ap.add_argument("--no-gather", action="store_true", help="leave out the two passes through the diagnostic library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure_all(a, a.child)))
        return
    cases = measure_all(a, "period")
    by = {c["case"].split("/", 1)[1]: c for c in cases}
    for label, switch in (() if a.no_gather else (("gather", "PCX_SRC_GATHER"), ("period_no_lds", "PCX_SRC_NO_LDS"))):
        diag = os.path.join(ROOT, "pothoscomms_amd", "libpcx_hip_diag.so")
        if not os.path.exists(diag):
            sys.exit("source_rate: %s is missing (make -C pothoscomms_amd/csrc diag)" % diag)
        env = dict(os.environ, PCX_HIP_LIBRARY=diag)
        env[switch] = "1"
        argv = [sys.executable, os.path.abspath(__file__), "--child", label, "--n", str(a.n), "--window", str(a.window), "--warmup", str(a.warmup),
                "--trials", str(a.trials)]
        r = subprocess.run(argv, env=env, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.exit("source_rate: the %s pass failed\n" % label + r.stdout[-2000:] + r.stderr[-2000:])
        other = json.loads(r.stdout.strip().splitlines()[-1])
        for g in other:
            g["time_over_period_form"] = round(g["call_ms"] / by[g["case"].split("/", 1)[1]]["call_ms"], 3)
        cases += other
    lines = ["| case | elements | period | in LDS | call ms | bytes written | bytes/s | spread | share of 8 TB/s | fill, same bytes: ms | fill bytes/s | "
             "its spread | time / fill | time / period form |", "|" + "---|" * 14]
    for c in cases:
        lines.append("| %s | %d | %d | %s | %.4f | %d | %.4g | %.4f | %.3f | %.4f | %.4g | %.4f | %.3f | %s |" % (
            c["case"], c["elements"], c["period"], "yes" if c["staged_in_lds"] else "no", c["call_ms"], c["bytes_written"], c["bytes_per_s"],
            c["spread"], c["share_of_hbm_peak"], c["fill_same_bytes_ms"], c["fill_bytes_per_s"], c["fill_spread"], c["time_over_fill"],
            ("%.3f" % c["time_over_period_form"]) if "time_over_period_form" in c else ""))
    text = "\n".join(lines) + "\n" + json.dumps({"metric": "source_rate", "cases": cases})
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
