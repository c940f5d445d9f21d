"""The rates of /comms/symbol_mapper, /comms/symbol_slicer, /comms/differential_encoder and /comms/differential_decoder on the device
at 64 Mi elements per call: a table, then one JSON line.

Cases: the mapper and the slicer at complex_float32, complex_int16 and float32 with maps of 2, 4, 16, 64 and 256 entries; the encoder's
SCAN plan at 2 and 256 symbols; the decoder; and each block once more with both pointers off the 16-byte grid ("unaligned").  Device-resident input and output (process_dev), hip events around as many back-to-back
calls as fill `--window` seconds, after `--warmup` calls; the median of `--trials` windows with their spread (slowest over fastest - 1).

Per case: elements/s; the bytes the algorithm must move (one read of the input, one write of the output) and, where the plan moves
more, the bytes it moves; for the slicer the vector operations it must issue per call (OPS below, per sample and map entry); the least
time either takes at the peaks of MI355X_MICROARCH.md (8 TB/s; 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz vector lane-operations/s);
which of the two bounds the case, and the share of that bound the measured time reaches.

Two baselines are measured in the same call, each window right after the case's own (alternating): the project's element-wise map
kernel (/comms/conjugate, complex_float32) moving the same number of bytes -- the yardstick for the memory-bound cases -- and once at
the end the restated loops on one host core (skipped without gcc).
    python tools/symbols_rate.py [--n 67108864] [--window 0.3] [--warmup 3] [--trials 5] [--out FILE]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                          # bytes/s
VALU_PEAK = 256 * 4 * 32 * 2.4e9           # vector lane-operations/s
TYPES = [("complex_float32", 8), ("complex_int16", 4), ("float32", 4)]
MAPS = [2, 4, 16, 64, 256]
# vector operations per sample and map entry: complex float32 two subtractions, two products, a sum, a compare and two selects; complex
# int16 two conversions more; float32 a subtraction (the absolute value is an operand modifier), a compare and two selects
OPS = {"complex_float32": 8, "complex_int16": 10, "float32": 4}

HOST_LOOPS = r"""
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
typedef struct { float re, im; } cf32;
typedef struct { int16_t re, im; } ci16;
#define MAP_LOOP(NAME, T) \
void NAME(const unsigned char *in, T *out, size_t n, const T *map, unsigned mask) \
{ \
    for (size_t i = 0; i < n; i++) out[i] = map[in[i] & mask]; \
}
#define SLICE_LOOP(NAME, T, DIST) \
void NAME(const T *in, unsigned char *out, size_t n, const T *map, size_t len) \
{ \
    for (size_t i = 0; i < n; i++) { \
        unsigned char best = 0; \
        float dist = FLT_MAX; \
        for (size_t j = 0; j < len; j++) { \
            const float d = DIST(map[j], in[i]); \
            if (d < dist) { dist = d; best = (unsigned char)j; } \
        } \
        out[i] = best; \
    } \
}
static inline float dist_cf32(cf32 m, cf32 x) { const float dr = m.re - x.re, di = m.im - x.im; return dr * dr + di * di; }
static inline float dist_ci16(ci16 m, ci16 x) { const float dr = (float)(m.re - x.re), di = (float)(m.im - x.im); return dr * dr + di * di; }
static inline float dist_f32(float m, float x) { return __builtin_fabsf(m - x); }
MAP_LOOP(host_map_complex_float32, cf32)
MAP_LOOP(host_map_complex_int16, ci16)
MAP_LOOP(host_map_float32, float)
SLICE_LOOP(host_slice_complex_float32, cf32, dist_cf32)
SLICE_LOOP(host_slice_complex_int16, ci16, dist_ci16)
SLICE_LOOP(host_slice_float32, float, dist_f32)
unsigned host_encode(const unsigned char *in, unsigned char *out, size_t n, uint32_t symbols, unsigned last)
{
    uint8_t l = (uint8_t)last;
    for (size_t i = 0; i < n; i++) { l = (uint8_t)((in[i] + l + symbols) % symbols); out[i] = l; }
    return l;
}
unsigned host_decode(const unsigned char *in, unsigned char *out, size_t n, uint32_t symbols, unsigned last)
{
    uint8_t l = (uint8_t)last;
    for (size_t i = 0; i < n; i++) { const uint8_t b = l; l = in[i]; out[i] = (uint8_t)((l - b + symbols) % symbols); }
    return l;
}
"""


def make_map(rng, tname, M):
    """a random map of M entries in the stream type's own layout"""
    shape = (M, 2) if tname.startswith("complex_") else (M,)
    if "float" in tname:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(-20000, 20000, shape, dtype=np.int64).astype(np.int16)


def host_rates(n, trials):
    """{case: elements/s} of the restated loops on one host core, None without a compiler"""
    if shutil.which("gcc") is None or n == 0:
        return None
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        src, lib = os.path.join(wd, "host_loops.c"), os.path.join(wd, "host_loops.so")
        with open(src, "w") as f:
            f.write(HOST_LOOPS)
        subprocess.check_call(["gcc", "-O3", "-fno-fast-math", "-shared", "-fPIC", src, "-o", lib])
        L = C.CDLL(lib)
        vp, sz = C.c_void_p, C.c_size_t
        for tname, _ in TYPES:
            getattr(L, "host_map_" + tname).argtypes = [vp, vp, sz, vp, C.c_uint]
            getattr(L, "host_slice_" + tname).argtypes = [vp, vp, sz, vp, sz]
        L.host_encode.argtypes = L.host_decode.argtypes = [vp, vp, sz, C.c_uint32, C.c_uint]
        rng = np.random.default_rng(1)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        y = np.zeros_like(b)

        def med(fn):
            times = []
            for _ in range(trials):
                t0 = time.perf_counter()
                fn()
                times.append(time.perf_counter() - t0)
            return round(n / sorted(times)[len(times) // 2], 1)
        for tname, _ in TYPES:
            hmap, hslice = getattr(L, "host_map_" + tname), getattr(L, "host_slice_" + tname)
            for M in MAPS:
                m = make_map(rng, tname, M)
                pts = np.zeros((n,) + m.shape[1:], m.dtype)
                out["mapper/%s/%d" % (tname, M)] = med(lambda: hmap(b.ctypes.data, pts.ctypes.data, n, m.ctypes.data, M - 1))
                if "float" in tname:                        # the slicer reads the mapped points with fresh noise, as on the device
                    pts += (rng.standard_normal(pts.shape) * 0.3).astype(np.float32)
                out["slicer/%s/%d" % (tname, M)] = med(lambda: hslice(pts.ctypes.data, y.ctypes.data, n, m.ctypes.data, M))
        for s in (2, 256):
            out["encoder/%d" % s] = med(lambda: L.host_encode(b.ctypes.data, y.ctypes.data, n, s, 0))
        out["decoder/2"] = med(lambda: L.host_decode(b.ctypes.data, y.ctypes.data, n, 2, 0))
    return out


def windows(torch, s, call, base, window, warmup, trials):
    """medians and spreads of `trials` alternating windows of the case and of the baseline: (t_case, spread_case, t_base, spread_base)"""
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


def entry(name, n, t, spread, tb, spread_b, must, moved, ops):
    t_mem, t_alu = must / HBM_PEAK, ops / VALU_PEAK
    bound = "vector issue" if t_alu > t_mem else "HBM"
    return {"case": name, "elements": n, "call_ms": round(t * 1e3, 4), "elements_per_s": round(n / t, 1), "spread": round(spread, 4),
            "bytes_must_move": must, "bytes_plan_moves": moved, "vector_ops_must_issue": ops, "bound": bound,
            "share_of_bound": round(max(t_mem, t_alu) / t, 3), "plan_bytes_per_s": round(moved / t, 1),
            "elementwise_same_bytes_ms": round(tb * 1e3, 4), "elementwise_spread": round(spread_b, 4),
            "time_over_elementwise": round(t / tb, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--host-elements", type=int, default=4 << 20, help="elements per call of the host loops (0: skip them)")
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("symbols_rate: no GPU")
    from pothoscomms_amd import device as dev
    n = a.n
    s = torch.cuda.current_stream()
    rng = np.random.default_rng(2)
    sym = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0")
    sym_out = torch.empty_like(sym)
    scratch_in = torch.zeros(n * 9 // 16 + 1, 2, dtype=torch.float32, device="cuda:0")       # the element-wise yardstick's buffers
    scratch_out = torch.empty_like(scratch_in)
    cases = []

    def baseline(nbytes):
        nel = max(1, nbytes // 16)                         # complex_float32: 8 bytes read and 8 written per element
        return lambda: dev.conj(scratch_in, dev.F32, out=scratch_out, n=nel, stream=s)

    for tname, es in TYPES:
        cplx = tname.startswith("complex_")
        tdt = {"float32": torch.float32, "int16": torch.int16}[tname.replace("complex_", "")]
        pts = torch.empty((n, 2) if cplx else (n,), dtype=tdt, device="cuda:0")
        for M in MAPS:
            m = make_map(rng, tname, M)
            mp, sl = dev.SymbolMapper(tname, m), dev.SymbolSlicer(tname, m)
            moved = n * (1 + es)
            t, sp, tb, spb = windows(torch, s, lambda: mp.process_dev(sym, pts, n, stream=s), baseline(moved), a.window, a.warmup, a.trials)
            cases.append(entry("mapper/%s/%d" % (tname, M), n, t, sp, tb, spb, moved, moved, 0))
            # the slicer's input is made anew for every case: this map's points for `sym`, on the float types with noise of one
            # sigma so that the distances are not trivial and every case sees the same distribution around its own map
            mp.process_dev(sym, pts, n, stream=s)
            x = pts + torch.randn_like(pts) * 0.3 if "float" in tname else pts
            t, sp, tb, spb = windows(torch, s, lambda: sl.process_dev(x, sym_out, n, stream=s), baseline(moved), a.window, a.warmup, a.trials)
            cases.append(entry("slicer/%s/%d" % (tname, M), n, t, sp, tb, spb, moved, moved, n * M * OPS[tname]))
            if M == 4:
                # both pointers off the 16-byte grid: the bytes start one byte in, the samples one element in
                k = n - 16
                t, sp, tb, spb = windows(torch, s, lambda: mp.process_dev(sym[1:], pts[1:], k, stream=s), baseline(k * (1 + es)), a.window,
                                         a.warmup, a.trials)
                cases.append(entry("mapper/%s/%d/unaligned" % (tname, M), k, t, sp, tb, spb, k * (1 + es), k * (1 + es), 0))
                t, sp, tb, spb = windows(torch, s, lambda: sl.process_dev(x[1:], sym_out[1:], k, stream=s), baseline(k * (1 + es)), a.window,
                                         a.warmup, a.trials)
                cases.append(entry("slicer/%s/%d/unaligned" % (tname, M), k, t, sp, tb, spb, k * (1 + es), k * (1 + es), k * M * OPS[tname]))
            mp.close()
            sl.close()
            del x
        del pts
    for symbols in (2, 256):
        enc = dev.DifferentialCoder(False, symbols)
        assert enc.plan() == 0
        t, sp, tb, spb = windows(torch, s, lambda: enc.process_dev(sym, sym_out, n, stream=s), baseline(2 * n), a.window, a.warmup, a.trials)
        cases.append(entry("encoder/%d" % symbols, n, t, sp, tb, spb, 2 * n, 3 * n, 0))          # the SCAN plan reads the input twice
        enc.close()
    dec = dev.DifferentialCoder(True, 2)
    t, sp, tb, spb = windows(torch, s, lambda: dec.process_dev(sym, sym_out, n, stream=s), baseline(2 * n), a.window, a.warmup, a.trials)
    cases.append(entry("decoder/2", n, t, sp, tb, spb, 2 * n, 2 * n, 0))
    k = n - 16                                             # input and output off the 16-byte grid by different amounts
    enc = dev.DifferentialCoder(False, 256)
    t, sp, tb, spb = windows(torch, s, lambda: enc.process_dev(sym[1:], sym_out[3:], k, stream=s), baseline(2 * k), a.window, a.warmup, a.trials)
    cases.append(entry("encoder/256/unaligned", k, t, sp, tb, spb, 2 * k, 3 * k, 0))
    enc.close()
    t, sp, tb, spb = windows(torch, s, lambda: dec.process_dev(sym[1:], sym_out[3:], k, stream=s), baseline(2 * k), a.window, a.warmup, a.trials)
    cases.append(entry("decoder/2/unaligned", k, t, sp, tb, spb, 2 * k, 2 * k, 0))
    dec.close()
    host = host_rates(a.host_elements, 3)
    lines = ["| case | call ms | elements/s | spread | bytes must move | bytes the plan moves | vector ops | bound | share of bound | "
             "element-wise, same bytes: ms | its spread | time / element-wise | one host core, elements/s |", "|" + "---|" * 13]
    for c in cases:
        h = (host or {}).get(c["case"])
        lines.append("| %s | %.4f | %.4g | %.4f | %d | %d | %d | %s | %.3f | %.4f | %.4f | %.3f | %s |" % (
            c["case"], c["call_ms"], c["elements_per_s"], c["spread"], c["bytes_must_move"], c["bytes_plan_moves"], c["vector_ops_must_issue"],
            c["bound"], c["share_of_bound"], c["elementwise_same_bytes_ms"], c["elementwise_spread"], c["time_over_elementwise"],
            "%.4g" % h if h else "not measured"))
    text = "\n".join(lines) + "\n" + json.dumps({"metric": "symbols_rate", "cases": cases, "host_one_core_elements_per_s": host})
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
