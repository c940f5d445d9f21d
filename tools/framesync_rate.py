"""The rate of /comms/frame_sync's search on the device: one JSON line.

Default widths (symbol width 20, data width 4) and the 13-symbol Barker code: W = 1040 samples per correlation, F = 1272.  Streams of
`--elements` device-resident elements of both types, three ways:
  silence   noise a hundred times under the input threshold: every offset is gated (two loads per offset)
  carrier   a constant carrier: every gate is open, every offset correlates over W samples (|L| = 5/13 W: nothing is declared)
  frames    a frame (sync word, header, 600 payload symbols) every 4 Ki samples of a stream of at most 1 Mi elements: the loop of calls a
            block makes, a call seeing at most `--slab` elements; a search call ends at the frame it finds, and what it correlated behind
            that frame (the rest of its piece) is correlated again by the next search call
silence and carrier are ONE call on the whole stream (its offsets correlated in pieces of 16 Ki, 32 Ki, ... 4 Mi offsets, each followed by
the scan, the finish kernel and one read-back): hip events around `--reps` calls,
the median of `--trials` windows with their spread (max / min - 1), the windows alternating with those of a device-to-device copy of the
same bytes.  frames is a host clock around the whole loop (every search call synchronises), the median of min(`--trials`, 3) runs.
offsets_per_s is offsets over time; macs_per_s counts the N W complex multiply-adds of the correlation where it runs (carrier: every
offset; silence: none); flops_per_s prices a sample at the 14 double operations of framesync.hip's inner loop.
    python tools/framesync_rate.py [--elements 4194304] [--slab 65536] [--reps 5] [--warmup 2] [--trials 5]
    python tools/framesync_rate.py --table profiles/framesync/framesync_rate.json
The second form touches no device: it prints the Markdown table of profiles/framesync/framesync_rate.md from the JSON line of a run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BARKER13 = (1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1)
FLOPS_PER_SAMPLE = 14                   # the rotation's step (6), sample times rotation (6), the sum (2): framesync.hip corr_span
FP64_PEAK = 78.6e12                     # vector double precision, MI355X data sheet


def median_spread(t):
    t = sorted(t)
    return t[len(t) // 2], t[-1] / t[0] - 1


def stream_of(kind, n, np_ct, seed=3):
    import framesync_model as M
    rng = np.random.default_rng(seed)
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 1e-4
    if kind == "silence":
        return noise.astype(np_ct), 0
    if kind == "carrier":
        return (0.8 * np.exp(1j * (0.3 + 0.01 * np.arange(n))) + noise).astype(np_ct), 0
    s = M.settings(sw=20, dw=4, preamble=BARKER13)
    period, x, frames = 4096, np.zeros(n, np.complex128), 0
    fr = M.frame(s, 600, M.qpsk(rng, 600))            # 1272 + 2400 samples
    for at in range(100, n - period, period):
        x[at:at + len(fr)] = fr
        frames += 1
    return (0.8 * x * np.exp(1j * (0.3 + 0.01 * np.arange(n))) + noise).astype(np_ct), frames


def time_case(dev, torch, dtype, kind, n, slab, reps, warmup, trials):
    np_ct = np.complex64 if dtype == "complex_float32" else np.complex128
    es = 8 if dtype == "complex_float32" else 16
    if kind == "frames":
        n = min(n, 1 << 20)
    xh, frames = stream_of(kind, n, np_ct)
    x = torch.from_numpy(xh.view(xh.real.dtype).reshape(-1, 2)).cuda()
    y, src = torch.empty_like(x), torch.empty_like(x)
    fs = dev.FrameSync(dtype, "PHASE", BARKER13)
    W, F = fs.geometry()[:2]
    s = torch.cuda.current_stream()

    def window(fn, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(count):
            fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3 / count
    copy = lambda: y.copy_(src)                                        # noqa: E731
    res = {"dtype": dtype, "case": kind, "elements": n, "bytes": n * es, "W": W, "F": F}
    if kind != "frames":
        def call():
            fs.activate()
            r = fs.process_dev(x, n, y, n, stream=s)
            assert (r.consumed, r.produced, r.labels) == (n - F + 1, 0, [])
        for _ in range(warmup):
            call()
            copy()
        torch.cuda.synchronize()
        t_call, t_copy = [], []
        for _ in range(trials):
            t_copy.append(window(copy, reps))
            t_call.append(window(call, reps))
        (tc, sc), (tk, sk) = median_spread(t_copy), median_spread(t_call)
        offsets = n - F + 1
        macs = offsets * W if kind == "carrier" else 0
        res.update(offsets=offsets, calls=1, frames=0, call_ms=round(tk * 1e3, 4), call_spread=round(sk, 4), copy_ms=round(tc * 1e3, 4), copy_spread=round(sc, 4),
                   offsets_per_s=round(offsets / tk), bytes_per_s=round(n * es / tk), copy_bytes_per_s=round(2 * n * es / tc), call_over_copy=round(tk / tc, 2),
                   macs=macs, macs_per_s=round(macs / tk), flops_per_s=round(macs * FLOPS_PER_SAMPLE / tk),
                   share_of_fp64_peak=round(macs * FLOPS_PER_SAMPLE / tk / FP64_PEAK, 4))
        fs.close()
        return res

    def loop():
        fs.activate()
        pos, calls, found, produced = 0, 0, 0, 0
        while True:
            n_in = min(slab, n - pos)
            r = fs.process_dev(x[pos:], n_in, y, n_in, stream=s)
            calls += 1
            found += bool(r.labels)
            produced += r.produced
            pos += r.consumed
            if r.consumed == 0 and r.produced == 0:
                return calls, found, produced
    for _ in range(max(1, warmup - 1)):
        calls, found, produced = loop()
    assert found == frames and produced == frames * 2400, "frames found: %d of %d, %d elements produced" % (found, frames, produced)
    torch.cuda.synchronize()
    times, t_copy = [], []
    for _ in range(min(trials, 3)):
        t_copy.append(window(copy, reps))
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    (tk, sk), (tc, sc) = median_spread(times), median_spread(t_copy)
    res.update(offsets=n, calls=calls, frames=frames, frames_found=found, produced=produced, slab=slab, call_ms=round(tk * 1e3, 4), call_spread=round(sk, 4), copy_ms=round(tc * 1e3, 4),
               copy_spread=round(sc, 4), offsets_per_s=round(n / tk), bytes_per_s=round(n * es / tk), copy_bytes_per_s=round(2 * n * es / tc),
               call_over_copy=round(tk / tc, 2), ms_per_call=round(tk * 1e3 / calls, 4))
    fs.close()
    return res


def table(path):
    P = json.loads(open(path).read().strip().splitlines()[-1])
    print("`python tools/framesync_rate.py` on one MI355X: %d elements per stream, symbol width 20, data width 4, the 13-symbol Barker code (W = 1040, "
          "F = 1272).  silence and carrier: one call on the whole stream, hip events around %d calls after %d warm-up calls, median of %d windows, "
          "spread = max / min - 1; frames: a frame every 4 Ki samples through the loop of calls (slabs of %d elements), host clock, median of %d runs.  "
          "`copy` is a device-to-device copy of the same bytes.  Made by `python tools/framesync_rate.py --table` from the JSON file beside it.\n"
          % (P["elements"], P["reps"], P["warmup"], P["trials"], P["slab"], min(P["trials"], 3)))
    print("| type | case | calls | frames | time ms (spread) | copy ms (spread) | time / copy | offsets / s | correlation MAC / s | double FLOP / s (share of 78.6 T) |")
    print("|" + "---|" * 10)
    for c in P["cases"]:
        print("| %s | %s | %d | %d | %.3f (%.3f) | %.4f (%.3f) | %.1f | %.3g | %s | %s |" % (
            c["dtype"], c["case"], c["calls"], c["frames"], c["call_ms"], c["call_spread"], c["copy_ms"], c["copy_spread"], c["call_over_copy"], c["offsets_per_s"],
            "%.3g" % c["macs_per_s"] if c.get("macs") else "-", "%.3g (%.3f)" % (c["flops_per_s"], c["share_of_fp64_peak"]) if c.get("macs") else "-"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", metavar="JSON")
    ap.add_argument("--elements", type=int, default=4 << 20)
    ap.add_argument("--slab", type=int, default=64 << 10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trials", type=int, default=5)
    a = ap.parse_args()
    if a.table:
        return table(a.table)
    import torch
    if not torch.cuda.is_available():
        sys.exit("framesync_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = [time_case(dev, torch, dtype, kind, a.elements, a.slab, a.reps, a.warmup, a.trials)
             for dtype in ("complex_float32", "complex_float64") for kind in ("silence", "carrier", "frames")]
    print(json.dumps({"metric": "framesync_rate", "elements": a.elements, "slab": a.slab, "reps": a.reps, "warmup": a.warmup, "trials": a.trials,
                      "tile": dev.FrameSync("complex_float32").geometry()[4], "cases": cases}))


if __name__ == "__main__":
    main()
