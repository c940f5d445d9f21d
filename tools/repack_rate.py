"""The rates of /comms/bits_to_symbols, /comms/symbols_to_bits, /comms/bytes_to_symbols and /comms/symbols_to_bytes on the device at
64 Mi input elements per call (one call slice: the largest whole number of tiles within 64 Mi): a table, then one JSON line.

Cases: every kind at widths 1, 2, 3, 7 and 8 in both bit orders, and each kind once more at width 3 with both pointers off the
16-byte grid ("unaligned").  Device-resident input and output (process_dev), hip events around as many back-to-back calls as fill
`--window` seconds, after `--warmup` calls; the median of `--trials` windows with their spread (slowest over fastest - 1).

These kernels touch every byte once, so a case is reported as bytes moved per second, input plus output.  The yardstick is a plain
device-to-device copy that moves the same number of bytes (half of them read, half written), timed in the same run, each window right
after the case's own (alternating).  Per case: the time over the copy's, and the share of the HBM peak of MI355X_MICROARCH.md (8 TB/s).
    python tools/repack_rate.py [--n 67108864] [--window 0.3] [--warmup 3] [--trials 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                          # bytes/s
KINDS = ["bits_to_symbols", "symbols_to_bits", "bytes_to_symbols", "symbols_to_bytes"]
WIDTHS = [1, 2, 3, 7, 8]
ORDERS = ["MSBit", "LSBit"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64 << 20, help="input elements per call at most (rounded down to whole tiles)")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("repack_rate: no GPU")
    from pothoscomms_amd import device as dev
    s = torch.cuda.current_stream()
    pad = 32
    src = torch.randint(0, 256, (a.n + pad,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(8 * a.n + pad, dtype=torch.uint8, device="cuda:0")
    copy_src = torch.randint(0, 256, (9 * a.n // 2 + pad,), dtype=torch.uint8, device="cuda:0")      # the yardstick's buffers
    copy_dst = torch.empty_like(copy_src)
    cases = []

    def measure(name, r, n, in_off, out_off):
        m = r.out_elems(n)
        moved = n + m
        half = moved // 2
        x, y, ca, cb = src[in_off:], dst[out_off:], copy_src[:half], copy_dst[:half]
        t, sp, tb, spb = windows(torch, s, lambda: r.process_dev(x, y, n, stream=s), lambda: cb.copy_(ca), a.window, a.warmup, a.trials)
        cases.append({"case": name, "in_elements": n, "out_elements": m, "call_ms": round(t * 1e3, 4), "bytes_moved": moved,
                      "bytes_per_s": round(moved / t, 1), "spread": round(sp, 4), "share_of_hbm_peak": round(moved / HBM_PEAK / t, 3),
                      "copy_same_bytes_ms": round(tb * 1e3, 4), "copy_bytes_per_s": round(2 * half / tb, 1), "copy_spread": round(spb, 4),
                      "time_over_copy": round(t / tb, 3)})

    for kind in KINDS:
        for w in WIDTHS:
            for order in ORDERS:
                r = dev.SymbolRepacker(kind, w, order)
                tile, _ = r.geometry()
                n = a.n // tile * tile
                measure("%s/%s/%d" % (kind, order, w), r, n, 0, 0)
                if w == 3 and order == "MSBit":
                    measure("%s/%s/%d/unaligned" % (kind, order, w), r, n, 1, 3)
                r.close()
    lines = ["| case | in elements | call ms | bytes moved | bytes/s | spread | share of 8 TB/s | copy, same bytes: ms | copy bytes/s | its spread | "
             "time / copy |", "|" + "---|" * 11]
    for c in cases:
        lines.append("| %s | %d | %.4f | %d | %.4g | %.4f | %.3f | %.4f | %.4g | %.4f | %.3f |" % (
            c["case"], c["in_elements"], c["call_ms"], c["bytes_moved"], c["bytes_per_s"], c["spread"], c["share_of_hbm_peak"],
            c["copy_same_bytes_ms"], c["copy_bytes_per_s"], c["copy_spread"], c["time_over_copy"]))
    text = "\n".join(lines) + "\n" + json.dumps({"metric": "repack_rate", "cases": cases})
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
