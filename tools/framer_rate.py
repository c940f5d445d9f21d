"""The rate of the framers' splice on the device: one JSON line.

uint8 (/comms/preamble_framer), complex_float32 and complex_float64 (/comms/frame_insert, with the header) streams of `--bytes` input
bytes, device-resident, framed three ways: frames of about 1 Ki and 64 Ki elements (a start label on the first and an end label on the
last element of each) and the dense case of a start label every 32 elements (on at most 16 Mi elements; bytes also with one every 80).  A call is a host plan, the
upload of its table and one kernel, so two times are given per case:
  device_ms   hip events around ONE call enqueued behind enough device-to-device copies of a 256 MiB buffer that the device is still
              busy while the host plans: the table's upload and the kernel alone
  call_ms     hip events around `--reps` back-to-back calls: what a caller sees, the host plan included where it is the longer part
each the median of `--trials` windows with their spread (max / min - 1), the windows alternating with those of a device-to-device copy
of the same output bytes (`copy_ms`, the comparison).  plan_ms is the host planner alone (pcx_framer_plan).  With PCX_HIP_LIBRARY set
to the diagnostic build, PCX_FRM_NO_LDS=1 makes every tile search its segments in global memory: the A/B partner of the staged table.
    python tools/framer_rate.py [--bytes 134217728] [--reps 10] [--warmup 2] [--trials 5]
    python tools/framer_rate.py --table product.json diag_staged.json diag_global.json
The second form touches no device: it prints the Markdown table of profiles/framer/framer_rate.md from the JSON lines of three runs (the
product library, the diagnostic library, the diagnostic library with PCX_FRM_NO_LDS=1).  Its segments column leaves the sentinel out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MALL_BYTES = 256 << 20                  # MI355X_MICROARCH.md
EVENT = np.dtype([("index", np.uint64), ("width", np.uint64), ("kind", np.uint32), ("length", np.uint32)])


def median_spread(t):
    t = sorted(t)
    return t[len(t) // 2], t[-1] / t[0] - 1


def events_of(_lib, n, kind):
    if kind.startswith("dense_"):
        step = int(kind[6:])
        ev = np.zeros(n // step, EVENT)
        ev["index"], ev["width"], ev["kind"] = np.arange(n // step, dtype=np.uint64) * step, 1, _lib.FRAME_START
    else:
        frame = {"frames_1Ki": 1000, "frames_64Ki": 65000}[kind]
        k = n // frame
        ev = np.zeros(2 * k, EVENT)
        ev["index"][0::2], ev["index"][1::2] = np.arange(k, dtype=np.uint64) * frame, np.arange(k, dtype=np.uint64) * frame + frame - 1
        ev["width"], ev["kind"][0::2], ev["kind"][1::2], ev["length"][0::2] = 1, _lib.FRAME_START, _lib.FRAME_END, frame & 0xFFFF
    return ev, ((_lib.FrameEvent * max(1, ev.size)).from_buffer(ev), ev.size)


def time_case(dev, _lib, torch, dtype, kind, nbytes, reps, warmup, trials):
    es = {"uint8": 1, "complex_float32": 8, "complex_float64": 16}[dtype]
    n = nbytes // es
    if kind.startswith("dense_"):
        n = min(n, 16 << 20)                                           # (half a million labels per call at the most)
    header = dtype != "uint8"
    pre = [1, 0, 1, 1, 0, 0, 1, 0] if not header else [1, 1, -1]
    f = dev.Framer(dtype, pre, 1 if not header else 20, header, padding=16)
    ev_np, ev = events_of(_lib, n, kind)
    plan = f.plan(n, 8 * n + 4096, ev, tables=False)[0]
    out_len = int(plan.out_len)
    assert plan.consumed == n and not plan.cut
    x = torch.randint(0, 255, (n * es,), dtype=torch.uint8, device="cuda:0")
    y = torch.empty(out_len * es, dtype=torch.uint8, device="cuda:0")
    src = torch.empty(out_len * es, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream()
    call = lambda: f.process_dev(x, n, ev, y, out_len, stream=s)      # noqa: E731
    copy = lambda: y.copy_(src)                                        # noqa: E731
    big_src, big_dst = (torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    filler = lambda: big_dst.copy_(big_src)                            # noqa: E731  (long enough that the host enqueues them faster than they run)
    t0 = time.perf_counter()
    for _ in range(3):
        f.plan(n, out_len, ev, tables=False)
    plan_s = (time.perf_counter() - t0) / 3
    for _ in range(warmup):
        call()
        copy()
    torch.cuda.synchronize()
    t_call, t_copy, t_dev = [], [], []

    def window(fn, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(count):
            fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / 1e3 / count
    for _ in range(trials):
        t_copy.append(window(copy, reps))
        t_call.append(window(call, reps))
        t_fill = window(filler, 4)
        for _ in range(int(2 * plan_s / t_fill) + 4):                  # keeps the device busy for twice the host plan
            filler()
        t_dev.append(window(call, 1))
    (tc, sc), (tk, sk), (td, sd) = median_spread(t_copy), median_spread(t_call), median_spread(t_dev)
    moved = (n + out_len) * es
    res = {"dtype": dtype, "case": kind, "in_elements": n, "out_elements": out_len, "events": int(ev_np.size), "segments": int(plan.n_segments),
           "table_bytes": int(plan.n_segments * 16 + plan.n_headers * 8), "plan_ms": round(plan_s * 1e3, 4),
           "copy_ms": round(tc * 1e3, 4), "copy_tb_per_s": round(2 * out_len * es / tc / 1e12, 3), "copy_spread": round(sc, 4),
           "device_ms": round(td * 1e3, 4), "device_tb_per_s": round(moved / td / 1e12, 3), "device_spread": round(sd, 4),
           "copy_time_over_device_time": round(tc / td, 3),
           "call_ms": round(tk * 1e3, 4), "call_spread": round(sk, 4), "copy_time_over_call_time": round(tc / tk, 3),
           "buffers": "fit the MALL" if moved <= MALL_BYTES else "stream from HBM"}
    f.close()
    return res


def table(paths):
    P, L, N = (json.loads(open(p).read().strip().splitlines()[-1]) for p in paths)
    print("`python tools/framer_rate.py` on one MI355X: %d input bytes per call (the dense case: at most 16 Mi elements), hip events, %d "
          "back-to-back calls per window after %d warm-up calls, median of %d windows, spread = max / min - 1 of the windows.  `device` is one "
          "call enqueued behind filler copies (table upload and kernel), `call` the back-to-back calls with the host plan, `copy` a "
          "device-to-device copy of the same output bytes; times in ms.  The last two columns are the diagnostic build's `device` time with the "
          "tile's table staged in LDS (up to %d segments) and with `PCX_FRM_NO_LDS=1` (every tile searches global memory).  Made by "
          "`python tools/framer_rate.py --table` from the three JSON files beside it.\n" % (P["input_bytes"], P["reps"], P["warmup"], P["trials"], P["lds_segments"]))
    print("| type | case | in elements | out elements | labels | segments | table bytes | plan | copy | device (spread) | device / copy | call (spread) "
          "| call / copy | staged (spread) | global (spread) |")
    print("|" + "---|" * 15)
    for p, l, n in zip(P["cases"], L["cases"], N["cases"]):
        print("| %s | %s | %d | %d | %d | %d | %d | %.3f | %.4f | %.4f (%.3f) | %.2f | %.3f (%.3f) | %.1f | %.4f (%.3f) | %.4f (%.3f) |" % (
            p["dtype"], p["case"], p["in_elements"], p["out_elements"], p["events"], p["segments"] - 1, p["table_bytes"], p["plan_ms"], p["copy_ms"],
            p["device_ms"], p["device_spread"], p["device_ms"] / p["copy_ms"], p["call_ms"], p["call_spread"], p["call_ms"] / p["copy_ms"],
            l["device_ms"], l["device_spread"], n["device_ms"], n["device_spread"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", nargs=3, metavar="JSON")
    ap.add_argument("--bytes", type=int, default=128 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trials", type=int, default=5)
    a = ap.parse_args()
    if a.table:
        return table(a.table)
    import torch
    if not torch.cuda.is_available():
        sys.exit("framer_rate: no GPU")
    from pothoscomms_amd import _lib, device as dev
    cases = [time_case(dev, _lib, torch, dtype, kind, a.bytes, a.reps, a.warmup, a.trials)
             for dtype in ("uint8", "complex_float32", "complex_float64") for kind in ("frames_1Ki", "frames_64Ki", "dense_32")]
    # bytes with a label every 80 elements: 372 segments in a tile, close under what a workgroup stages
    cases.append(time_case(dev, _lib, torch, "uint8", "dense_80", a.bytes, a.reps, a.warmup, a.trials))
    tile, lds = dev.Framer.geometry()
    print(json.dumps({"metric": "framer_rate", "input_bytes": a.bytes, "reps": a.reps, "warmup": a.warmup, "trials": a.trials, "tile_bytes": tile,
                      "lds_segments": lds, "library": "diag" if os.environ.get("PCX_HIP_LIBRARY") else "product", "no_lds": os.environ.get("PCX_FRM_NO_LDS", ""),
                      "cases": cases}))


if __name__ == "__main__":
    main()
