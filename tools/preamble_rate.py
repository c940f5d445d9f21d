"""The rate of /comms/preamble_correlator on the device at 64 Mi symbols per call: one JSON line.

Preambles of 32, 64, 256 and 1024 symbols with 1 and 8 active bit planes (a 0/1 preamble, and one of full bytes), device-resident
input (process_dev without the forwarded copy, then with it), hip events around `--reps` back-to-back calls after `--warmup` calls,
median of `--trials` windows with their spread.  Each entry gives Gsymbol/s, the vector operations and the bytes the plan needs per
position, computed from the shapes below, and which of the two bounds the call against the peaks of MI355X_MICROARCH.md.  For scale,
in the same run and alternating with the kernel: a device-to-device copy of the same bytes, and this project's own restatement of
the reference loop, compiled -O3, on one host core (skipped without gcc).
    python tools/preamble_rate.py [--n 67108864] [--reps 10] [--warmup 3] [--trials 5]
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                       # bytes/s, MI355X_MICROARCH.md
VALU_PEAK = 256 * 4 * 32 * 2.4e9        # lane operations/s: 256 CUs x 4 SIMD-32 at 2.4 GHz (157.3 TFLOPS / 2)
LENGTHS = [32, 64, 256, 1024]
TILE, WAVE, LANE_POS = 4096, 64, 16

HOST_LOOP = r"""
#include <stddef.h>
#include <stdint.h>
/* the reference's loop: the number of positions within the threshold */
size_t host_loop(const unsigned char *pre, size_t P, unsigned threshold, const unsigned char *in, size_t n)
{
    size_t hits = 0;
    if (n <= P) return 0;
    for (size_t i = 0; i < n - P; i++) {
        unsigned dist = 0;
        for (size_t k = 0; k < P; k++) dist += (unsigned)__builtin_popcount(pre[k] ^ in[i + k]);
        hits += dist <= threshold;
    }
    return hits;
}
"""


def plan_counts(P, planes, copy):
    """(vector lane operations, HBM bytes) per position of the PLANES plan as built (preamble.hip)"""
    staged = (TILE + P - 1) / TILE                  # staged bytes per position
    ops = 0.0
    ops += staged * 1.5                             # staging: a 16-byte load and LDS store per 16 bytes, address arithmetic
    ops += staged * (1 + 4 * planes)                # plane split per byte: an LDS read, and per plane and / compare / two moves of the ballot
    if planes < 8:
        ops += staged * (2.5 + 0.5 + 1) + 4         # prefix: mask + 2 popcounts per byte amortised, the scan, the stores; 2 reads + sub + add
    kfull, tail = P // 32, 1 if P % 32 else 0
    pairs = kfull * 2 + tail * 3                    # xor + bcnt per 32 symbols, + and on the masked tail
    chunks = kfull // 4 + (kfull % 4) // 2 + kfull % 2 + tail
    windows = (kfull + tail) + chunks * (LANE_POS - 1) / LANE_POS        # one alignbit (and one LDS word) per window
    ops += planes * (pairs + 2 * windows)
    ops += 3                                        # compare, ballot, mask word
    byts = staged + 1 / 8 + (1 if copy else 0)      # input with its halo, the match bits, the forwarded byte
    return round(ops, 2), round(byts, 3)


def host_rate(P, planes, n, trials):
    """Gsymbol/s of the reference loop on one host core, None without a compiler"""
    if shutil.which("gcc") is None:
        return None
    import numpy as np
    with tempfile.TemporaryDirectory() as wd:
        src, lib = os.path.join(wd, "host_loop.c"), os.path.join(wd, "host_loop.so")
        with open(src, "w") as f:
            f.write(HOST_LOOP)
        subprocess.check_call(["gcc", "-O3", "-shared", "-fPIC", src, "-o", lib])
        L = C.CDLL(lib)
        L.host_loop.restype = C.c_size_t
        L.host_loop.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t]
        rng = np.random.default_rng(1)
        pre = rng.integers(0, 2 if planes == 1 else 256, P, dtype=np.uint8)
        x = rng.integers(0, 2 if planes == 1 else 256, n, dtype=np.uint8)
        times = []
        for _ in range(trials):
            t0 = time.perf_counter()
            L.host_loop(pre.ctypes.data, P, 0, x.ctypes.data, n)
            times.append(time.perf_counter() - t0)
        times.sort()
        return round((n - P) / times[len(times) // 2] / 1e9, 5)


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


def time_case(dev, torch, P, planes, n, reps, warmup, trials, host_n):
    import numpy as np
    rng = np.random.default_rng(10 * P + planes)
    top = 2 if planes == 1 else 256
    pre = rng.integers(0, top, P, dtype=np.uint8)
    pre[:8] |= 1 if planes == 1 else (1 << np.arange(8)).astype(np.uint8)
    x = torch.randint(0, top, (n,), dtype=torch.uint8, device="cuda:0")
    y = torch.empty_like(x)
    cap = 1 << 20
    idx = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    thr = P // 4 if planes == 1 else 3 * P              # a few matches per million positions at most
    h = dev.PreambleCorrelator(pre, threshold=thr)
    s = torch.cuda.current_stream()
    (t, sp), (tc, spc), (td, _) = windows_of(torch, [lambda: h.process_dev(x, n, idx, cap, counts, stream=s),
                                                      lambda: h.process_dev(x, n, idx, cap, counts, out=y, stream=s),
                                                      lambda: y.copy_(x)], reps, warmup, trials)
    npos, nm = counts.tolist()
    ops, byts = plan_counts(P, planes, False)
    t_ops, t_bytes = npos * ops / VALU_PEAK, npos * byts / HBM_PEAK
    host = host_rate(P, planes, host_n, 3) if host_n else None
    rate = npos / t / 1e9
    return {"P": P, "planes": planes, "plan": "PLANES" if h.plan() == 0 else "BYTES", "positions": npos, "matches": nm, "call_ms": round(t * 1e3, 4),
            "gsym_per_s": round(rate, 2), "spread": round(sp, 4), "with_copy_ms": round(tc * 1e3, 4), "with_copy_gsym_per_s": round(npos / tc / 1e9, 2),
            "with_copy_spread": round(spc, 4), "ops_per_position": ops, "bytes_per_position": byts, "bound": "operations" if t_ops > t_bytes else "bytes",
            "share_of_bound": round(max(t_ops, t_bytes) / t, 3), "d2d_copy_ms": round(td * 1e3, 4), "ratio_to_copy": round(td / t, 3),
            "host_one_core_gsym_per_s": host, "ratio_to_host": None if not host else round(rate / host, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--host-symbols", type=int, default=1 << 20, help="symbols per call of the host loop (0: skip it)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("preamble_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = [time_case(dev, torch, P, planes, a.n, a.reps, a.warmup, a.trials, a.host_symbols) for planes in (1, 8) for P in LENGTHS]
    print(json.dumps({"metric": "preamble_rate", "symbols": a.n, "cases": cases}))


if __name__ == "__main__":
    main()
