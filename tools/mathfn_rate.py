"""The rates of the exp, log, pow, root and trigonometric maps on the device at 64 Mi elements per call: one JSON line.

Every case is pcx_mathfn_dev / pcx_mathfn_param_dev on device-resident tensors (device.math_fn), timed against a device-to-device
copy (tensor.copy_) of the same input in the same alternating windows: hip events around `--reps` back-to-back calls after `--warmup`
calls, median of `--trials` windows with their spread (max / min - 1).  A map reads its input and writes as many bytes, which is
what the copy does, so `time_ratio` = 1 is a map at the copy's rate and anything above it is what the arithmetic costs; `gelem_per_s`
is the rate that matters where the arithmetic binds.  Each entry says whether its tensors fit the 256 MiB of MALL (then the
repetitions of a window find them there: not a cold rate) or stream from HBM.  The cases: one cheap function (sqrt, and rsqrt, whose
float32 form is single precision), mid ones (exp, log10, sigmoid) and dear ones (pow, tan), in both types; inputs are uniform on
[0.5, 20.5], inside every one of these functions' domains (large trigonometric arguments are not timed).
    python tools/mathfn_rate.py [--n 67108864] [--reps 50] [--warmup 3] [--trials 7] [--table profiles/mathfn/mathfn_rate.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.threshold_rate import MALL_BYTES, windows_of  # noqa: E402

CASES = [("SQRT", None), ("RSQRT", None), ("EXP", None), ("LOG10", None), ("SIGMOID", None), ("TAN", None), ("POW", 1.5)]


def table(result):
    rows = ["| case | bytes per call | call ms | Gelem/s | TB/s | spread | copy ms | copy TB/s | copy spread | time / copy | tensors |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in result["cases"]:
        rows.append("| %s | %d | %.4f | %.1f | %.3f | %.4f | %.4f | %.3f | %.4f | %.3f | %s |" % (
            c["case"], c["bytes_moved"], c["call_ms"], c["gelem_per_s"], c["tb_per_s"], c["spread"], c["d2d_copy_ms"], c["d2d_copy_tb_per_s"], c["d2d_copy_spread"],
            c["time_ratio"], c["tensors"]))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--table", default=None, help="also write the cases as a markdown table to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mathfn_rate: no GPU")
    from pothoscomms_amd import device as dev
    s = torch.cuda.current_stream()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    cases = []
    for dtype in ("float32", "float64"):
        x = (torch.rand(a.n, device="cuda:0", generator=g, dtype=torch.float32) * 20 + 0.5).to(getattr(torch, dtype))
        y, dst = torch.empty_like(x), torch.empty_like(x)
        moved = 2 * x.numel() * x.element_size()
        for fn, p in CASES:
            (t, sp), (tcopy, spcopy) = windows_of(torch, [lambda: dev.math_fn(fn, x, p, out=y, stream=s), lambda: dst.copy_(x)], a.reps, a.warmup, a.trials)
            cases.append({"case": "%s%s %s" % (fn.lower(), "" if p is None else " %g" % p, dtype), "bytes_moved": moved, "call_ms": round(t * 1e3, 4),
                          "gelem_per_s": round(a.n / t / 1e9, 2), "tb_per_s": round(moved / t / 1e12, 3), "spread": round(sp, 4),
                          "d2d_copy_ms": round(tcopy * 1e3, 4), "d2d_copy_tb_per_s": round(moved / tcopy / 1e12, 3), "d2d_copy_spread": round(spcopy, 4),
                          "time_ratio": round(t / tcopy, 3), "tensors": "fit the MALL" if 3 * moved // 2 <= MALL_BYTES else "stream from HBM"})
        del x, y, dst
    result = {"metric": "mathfn_rate", "elements": a.n, "reps": a.reps, "warmup": a.warmup, "trials": a.trials, "cases": cases}
    print(json.dumps(result))
    if a.table:
        with open(a.table, "w") as f:
            f.write(table(result) + "\n")


if __name__ == "__main__":
    main()
