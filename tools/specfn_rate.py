"""The rates of the special-function maps on the device at 64 Mi elements per call: one JSON line.

Every case is pcx_specfn_dev, pcx_beta_dev or pcx_modf_dev on device-resident tensors (device.special_fn, device.beta, device.modf),
timed against a device-to-device copy (tensor.copy_) of one input in the same alternating windows, as tools/mathfn_rate.py does: hip
events around `--reps` back-to-back calls after `--warmup` calls, median of `--trials` windows with their spread (max / min - 1).
One process, one device.  A unary map moves what the copy moves (one read, one write), so `time_ratio` = 1 is a map at the copy's
rate; beta reads two streams and modf writes two, 1.5 times the copy's bytes, which `bytes_moved` and `tb_per_s` account for.
`gelem_per_s` is the rate that matters where the arithmetic binds.  Inputs are uniform on [0.5, 20.5]: inside every function's
domain, where gamma and erfc neither overflow nor underflow in either type.
    python tools/specfn_rate.py [--n 67108864] [--reps 20] [--warmup 2] [--trials 5] [--table profiles/specfn/specfn_rate.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mathfn_rate import table  # noqa: E402
from tools.threshold_rate import MALL_BYTES, windows_of  # noqa: E402

CASES = ["GAMMA", "LNGAMMA", "ERF", "ERFC", "BETA", "MODF"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--table", default=None, help="also write the cases as a markdown table to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("specfn_rate: no GPU")
    from pothoscomms_amd import device as dev
    s = torch.cuda.current_stream()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    cases = []
    for dtype in ("float32", "float64"):
        x = (torch.rand(a.n, device="cuda:0", generator=g, dtype=torch.float32) * 20 + 0.5).to(getattr(torch, dtype))
        x2 = (torch.rand(a.n, device="cuda:0", generator=g, dtype=torch.float32) * 20 + 0.5).to(getattr(torch, dtype))
        y, y2, dst = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        one = x.numel() * x.element_size()
        for fn in CASES:
            call = {"BETA": lambda: dev.beta(x, x2, out=y, stream=s), "MODF": lambda: dev.modf(x, out_int=y, out_frac=y2, stream=s)}.get(
                fn, lambda: dev.special_fn(fn, x, out=y, stream=s))
            moved = (3 if fn in ("BETA", "MODF") else 2) * one
            (t, sp), (tcopy, spcopy) = windows_of(torch, [call, lambda: dst.copy_(x)], a.reps, a.warmup, a.trials)
            cases.append({"case": "%s %s" % (fn.lower(), dtype), "bytes_moved": moved, "call_ms": round(t * 1e3, 4),
                          "gelem_per_s": round(a.n / t / 1e9, 2), "tb_per_s": round(moved / t / 1e12, 3), "spread": round(sp, 4),
                          "d2d_copy_ms": round(tcopy * 1e3, 4), "d2d_copy_tb_per_s": round(2 * one / tcopy / 1e12, 3), "d2d_copy_spread": round(spcopy, 4),
                          "time_ratio": round(t / tcopy, 3), "tensors": "fit the MALL" if moved + one <= MALL_BYTES else "stream from HBM"})
        del x, x2, y, y2, dst
    result = {"metric": "specfn_rate", "elements": a.n, "reps": a.reps, "warmup": a.warmup, "trials": a.trials, "cases": cases}
    print(json.dumps(result))
    if a.table:
        with open(a.table, "w") as f:
            f.write(table(result) + "\n")


if __name__ == "__main__":
    main()
