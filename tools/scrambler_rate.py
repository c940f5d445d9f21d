"""The rate of /comms/scrambler and /comms/descrambler on the device at 64 Mi bits per call: one JSON line.

Additive, multiplicative scrambler and multiplicative descrambler at the polynomials 0x19, 0x11021 and 0x8000000000000003 (all SCAN),
device-resident input and output (process_dev), hip events around `--reps` back-to-back calls after `--warmup` calls, median of
`--trials` windows with their spread.  Each entry: Gbit/s and the share of the HBM roof at the bytes the plan moves per bit at 8 TB/s
(additive: one read and one write, 2 B; multiplicative: the input is read twice, 3 B).  For scale the same loop -- this project's own
three-line restatement of the bit step, compiled -O3 -- is timed on one host core of the same box (skipped without g++).
    python tools/scrambler_rate.py [--n 67108864] [--reps 10] [--warmup 3] [--trials 5]
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

HBM_PEAK = 8.0e12     # bytes/s, MI355X_MICROARCH.md
KINDS = {"additive": (False, "additive"), "scrambler": (False, "multiplicative"), "descrambler": (True, "multiplicative")}
POLYS = [("0x19", 0x19, 0x9), ("0x11021", 0x11021, 0xACE1), ("bit63", 0x8000000000000003, 0x1234567)]

HOST_LOOP = r"""
#include <stddef.h>
#include <stdint.h>
/* kind 0 additive, 1 multiplicative scrambler, 2 multiplicative descrambler; returns the register */
uint64_t host_loop(const unsigned char *in, unsigned char *out, size_t n, uint64_t data, uint64_t polynomial, uint64_t mask, int kind)
{
    for (size_t i = 0; i < n; i++) {
        const unsigned char b = in[i] & 1;
        data <<= 1;
        const unsigned char ret = (data & mask) != 0;
        if (ret) data ^= polynomial;
        const unsigned char o = b ^ ret;
        if (kind == 1) data = (data & ~(uint64_t)1) | o;
        else if (kind == 2) data = (data & ~(uint64_t)1) | b;
        out[i] = o;
    }
    return data;
}
"""


def host_rates(n, trials):
    """{kind/poly: Gbit/s} of the bit loop on one host core, None without a compiler"""
    if shutil.which("gcc") is None:
        return None
    import numpy as np
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        src, lib = os.path.join(wd, "host_loop.c"), os.path.join(wd, "host_loop.so")
        with open(src, "w") as f:
            f.write(HOST_LOOP)
        subprocess.check_call(["gcc", "-O3", "-shared", "-fPIC", src, "-o", lib])
        L = C.CDLL(lib)
        L.host_loop.restype = C.c_uint64
        L.host_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
        x = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
        y = np.zeros_like(x)
        for k, kind in enumerate(KINDS):
            for pname, poly, seed in POLYS:
                top = poly.bit_length() - 1
                mask = ((1 << 64) - 1) & ~((1 << top) - 1)
                times = []
                for _ in range(trials):
                    t0 = time.perf_counter()
                    L.host_loop(x.ctypes.data, y.ctypes.data, n, seed, poly | 1, mask, k)
                    times.append(time.perf_counter() - t0)
                times.sort()
                out["%s/%s" % (kind, pname)] = round(n / times[len(times) // 2] / 1e9, 4)
    return out


def time_case(dev, torch, kind, pname, poly, seed, n, reps, warmup, trials):
    descramble, mode = KINDS[kind]
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0")
    y = torch.empty_like(x)
    h = dev.Scrambler(descramble, mode, poly, seed)
    plan = h.plan()
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
    per_bit = 2 if kind == "additive" else 3
    return {"kind": kind, "poly": pname, "plan": "SCAN" if plan == 0 else "SERIAL", "bits": n, "call_ms": round(t * 1e3, 4),
            "gbit_per_s": round(n / t / 1e9, 2), "bytes_per_bit": per_bit, "hbm_roof_share": round(n * per_bit / t / HBM_PEAK, 3),
            "spread": round(times[-1] / times[0] - 1, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--host-bits", type=int, default=16 << 20, help="bits per call of the host loop (0: skip it)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("scrambler_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = [time_case(dev, torch, kind, pname, poly, seed, a.n, a.reps, a.warmup, a.trials) for kind in KINDS for pname, poly, seed in POLYS]
    host = host_rates(a.host_bits, 3) if a.host_bits else None
    print(json.dumps({"metric": "scrambler_rate", "cases": cases, "host_one_core_gbit_per_s": host}))


if __name__ == "__main__":
    main()
