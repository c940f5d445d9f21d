"""The rates of the comparator, bitwise, byte-order and const-arithmetic maps on the device at 64 Mi elements per call: one JSON line.

Every case is a `_dev` call on device-resident tensors, timed against a device-to-device copy (tensor.copy_) of the case's first
input in the same alternating windows: hip events around `--reps` back-to-back calls after `--warmup` calls, median of `--trials`
windows with their spread (max / min - 1).  A map is a stream of its inputs plus its output, the copy a stream of twice its tensor:
the case's bytes over the copy's bytes is the ratio of times a map at the copy's rate would show (`expected_time_ratio`), and
`excess` is how far the measured ratio lies above it -- a finding where it exceeds the copy's own spread.  Each entry says whether
its tensors fit the 256 MiB of MALL (then the repetitions of a window find them there: not a cold rate) or stream from HBM.
Two orderings are measured in windows of their own: the float32 comparator (9 bytes per element) against /comms/arithmetic ADD on
the same inputs (12), and the one-pass XOR of eight inputs (9 streams) against seven two-input folds through the output (21).
    python tools/logic_rate.py [--n 67108864] [--reps 100] [--warmup 3] [--trials 7] [--table profiles/logic/logic_rate.md]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.threshold_rate import MALL_BYTES, windows_of  # noqa: E402

SC = {"float64": 0, "float32": 1, "int64": 2, "int32": 3, "int16": 4, "int8": 5, "uint64": 6, "uint32": 7, "uint16": 8, "uint8": 9}
WIDTH = {"float64": 8, "float32": 4, "int64": 8, "int32": 4, "int16": 2, "int8": 1, "uint64": 8, "uint32": 4, "uint16": 2, "uint8": 1}


def operand(torch, dtype, n, per, seed):
    """n elements of `per` scalars: floats of ordinary size, integers over their whole range (no zeros for the divisions' sake)"""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    if dtype.startswith("float"):
        return ((torch.rand(n * per, device="cuda:0", generator=g, dtype=torch.float32) * 200 - 100) + 0.5).to(getattr(torch, dtype))
    raw = torch.randint(1, 256, (n * per * WIDTH[dtype],), device="cuda:0", generator=g, dtype=torch.uint8)
    return raw


def cases_of(dev, torch, n):
    """(name, bytes the map moves, tensors it holds, the call)"""
    s = torch.cuda.current_stream()
    out = []

    def add(name, moved, tensors, fn):
        out.append((name, moved, tensors, fn))

    for dtype in ("float32", "float64", "int16", "uint8"):
        w = WIDTH[dtype]
        a, b = operand(torch, dtype, n, 1, 1), operand(torch, dtype, n, 1, 2)
        y = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        add("compare > %s" % dtype, (2 * w + 1) * n, [a, b, y], lambda a=a, b=b, y=y, sc=SC[dtype]: dev.compare(">", a, b, scalar=sc, out=y, n=n, stream=s))
        add("compare_const > %s" % dtype, (w + 1) * n, [a, y], lambda a=a, y=y, sc=SC[dtype]: dev.compare_const(">", a, 0, scalar=sc, out=y, n=n, stream=s))
    for dtype in ("uint8", "uint64"):
        w = WIDTH[dtype]
        a, b = operand(torch, dtype, n, 1, 3), operand(torch, dtype, n, 1, 4)
        y = torch.empty_like(a)
        add("bitwise NOT %s" % dtype, 2 * w * n, [a, y], lambda a=a, y=y, sc=SC[dtype]: dev.bitwise("NOT", [a], scalar=sc, out=y, n=n, stream=s))
        add("bitwise XOR 2 inputs %s" % dtype, 3 * w * n, [a, b, y], lambda a=a, b=b, y=y, sc=SC[dtype]: dev.bitwise("XOR", [a, b], scalar=sc, out=y, n=n, stream=s))
        add("bitwise_const XOR %s" % dtype, 2 * w * n, [a, y], lambda a=a, y=y, sc=SC[dtype]: dev.bitwise_const("XOR", a, 0x5A, scalar=sc, out=y, n=n, stream=s))
    for dtype in ("int8", "int16", "int64"):
        a = operand(torch, dtype, n, 1, 5)
        y = torch.empty_like(a)
        add("bitshift >> %s" % dtype, 2 * WIDTH[dtype] * n, [a, y], lambda a=a, y=y, sc=SC[dtype]: dev.bitshift(False, a, 3, scalar=sc, out=y, n=n, stream=s))
    for w, dtype in ((2, "uint16"), (4, "uint32"), (8, "uint64")):
        a = operand(torch, dtype, n, 1, 6)
        y = torch.empty_like(a)
        add("byteswap %d bytes" % w, 2 * w * n, [a, y], lambda a=a, y=y, w=w: dev.byteswap(a, width=w, out=y, n=n, stream=s))
    for op, dtype, cplx in (("X*K", "float32", False), ("X+K", "int8", False), ("X/K", "int32", False), ("X/K", "int64", False), ("K/X", "int64", False),
                            ("X*K", "float32", True), ("X/K", "float32", True), ("X/K", "float64", True), ("X/K", "int16", True)):
        per = 2 if cplx else 1
        a = operand(torch, dtype, n, per, 7)
        y = torch.empty_like(a)
        k = (3 - 2j) if cplx else 7
        add("arith_const %s %s%s" % (op, "complex_" if cplx else "", dtype), 2 * per * WIDTH[dtype] * n, [a, y],
            lambda a=a, y=y, op=op, k=k, cplx=cplx, sc=SC[dtype]: dev.arith_const(op, a, k, cplx, scalar=sc, out=y, n=n, stream=s))
    return out


def nbytes(t):
    return t.numel() * t.element_size()


def entry(name, moved, tensors, t, sp, tcopy, spcopy):
    copy_bytes = 2 * nbytes(tensors[0])
    expected = moved / copy_bytes
    held = sum(nbytes(x) for x in tensors)
    return {"case": name, "bytes_moved": moved, "call_ms": round(t * 1e3, 4), "tb_per_s": round(moved / t / 1e12, 3), "spread": round(sp, 4),
            "d2d_copy_ms": round(tcopy * 1e3, 4), "d2d_copy_tb_per_s": round(copy_bytes / tcopy / 1e12, 3), "d2d_copy_spread": round(spcopy, 4),
            "time_ratio": round(t / tcopy, 3), "expected_time_ratio": round(expected, 3), "excess": round(t / tcopy / expected - 1, 4),
            "tensors": "fit the MALL" if held <= MALL_BYTES else "stream from HBM"}


def orderings(dev, torch, n, reps, warmup, trials):
    s = torch.cuda.current_stream()
    a, b = operand(torch, "float32", n, 1, 11), operand(torch, "float32", n, 1, 12)
    y8, y32 = torch.empty(n, dtype=torch.uint8, device="cuda:0"), torch.empty_like(a)
    (tc, sc_), (ta, sa) = windows_of(torch, [lambda: dev.compare(">", a, b, scalar=SC["float32"], out=y8, n=n, stream=s),
                                             lambda: dev.arith("ADD", a, b, False, scalar=SC["float32"], out=y32, n=n, stream=s)], reps, warmup, trials)
    first = {"compare_f32_ms": round(tc * 1e3, 4), "compare_f32_spread": round(sc_, 4), "arith_add_f32_ms": round(ta * 1e3, 4), "arith_add_f32_spread": round(sa, 4),
             "compare_over_add": round(tc / ta, 3), "bytes_ratio": 0.75, "tensors": "fit the MALL" if 13 * n <= MALL_BYTES else "stream from HBM"}
    del a, b, y8, y32
    xs = [operand(torch, "uint32", n, 1, 20 + i) for i in range(8)]
    acc = torch.empty_like(xs[0])

    def pairwise():
        dev.bitwise("XOR", [xs[0], xs[1]], scalar=SC["uint32"], out=acc, n=n, stream=s)
        for x in xs[2:]:
            dev.bitwise("XOR", [acc, x], scalar=SC["uint32"], out=acc, n=n, stream=s)

    (t1, s1), (t7, s7) = windows_of(torch, [lambda: dev.bitwise("XOR", xs, scalar=SC["uint32"], out=acc, n=n, stream=s), pairwise], reps, warmup, trials)
    second = {"one_pass_8_inputs_ms": round(t1 * 1e3, 4), "one_pass_spread": round(s1, 4), "one_pass_tb_per_s": round(9 * 4 * n / t1 / 1e12, 3),
              "seven_pairwise_folds_ms": round(t7 * 1e3, 4), "pairwise_spread": round(s7, 4), "one_pass_over_pairwise": round(t1 / t7, 3), "streams_ratio": round(9 / 21, 3),
              "tensors": "fit the MALL" if 9 * 4 * n <= MALL_BYTES else "stream from HBM"}
    return {"compare_f32_against_arith_add_f32": first, "xor_8_inputs_one_pass_against_pairwise": second}


def table(result):
    rows = ["| case | bytes per call | call ms | TB/s | spread | copy ms | copy TB/s | copy spread | time / copy | expected | excess | tensors |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in result["cases"]:
        rows.append("| %s | %d | %.4f | %.3f | %.4f | %.4f | %.3f | %.4f | %.3f | %.3f | %+.4f | %s |" % (
            c["case"], c["bytes_moved"], c["call_ms"], c["tb_per_s"], c["spread"], c["d2d_copy_ms"], c["d2d_copy_tb_per_s"], c["d2d_copy_spread"], c["time_ratio"],
            c["expected_time_ratio"], c["excess"], c["tensors"]))
    rows.append("")
    for name, o in result["orderings"].items():
        rows.append("**%s**: %s" % (name, ", ".join("%s = %s" % kv for kv in o.items())))
        rows.append("")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--table", default=None, help="also write the cases as a markdown table to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("logic_rate: no GPU")
    from pothoscomms_amd import device as dev
    cases = []
    pending = cases_of(dev, torch, a.n)
    while pending:
        name, moved, tensors, fn = pending.pop(0)
        dst = torch.empty_like(tensors[0])
        (t, sp), (tcopy, spcopy) = windows_of(torch, [fn, lambda: dst.copy_(tensors[0])], a.reps, a.warmup, a.trials)
        cases.append(entry(name, moved, tensors, t, sp, tcopy, spcopy))
        del dst, tensors, fn
    result = {"metric": "logic_rate", "elements": a.n, "reps": a.reps, "warmup": a.warmup, "trials": a.trials, "cases": cases,
              "orderings": orderings(dev, torch, a.n, a.reps, a.warmup, a.trials)}
    print(json.dumps(result))
    if a.table:
        with open(a.table, "w") as f:
            f.write(table(result) + "\n")


if __name__ == "__main__":
    main()
