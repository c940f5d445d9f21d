#!/usr/bin/env python3
"""Generate tests/golden/ref_digests.json: digests of the compiled reference's outputs on the seeded cases of ref_cases.py.

Run where oracle/_ref can be built (it needs the reference sources):
    make -C oracle all _ref && python tests/golden/make_ref_digests.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import oracle as o  # noqa: E402
from tests.golden import ref_cases as rc  # noqa: E402


def main():
    R = o.ref()
    if R is None:
        raise SystemExit("oracle/_ref is not built")
    out = {}
    for n in rc.FFT_SIZES:
        for key, x, inv in rc.fft_cases(n):
            out[key] = rc.digest(o.ref_fft(x, n, inv))
    out["atan2"] = rc.digest(np.array([R.ref_fxpt_atan2(y, x) for y, x in rc.atan2_pairs()], np.int64))
    for key, op, a, b, cplx in rc.arith_cases(o):
        out[key] = rc.digest(o.ref_arith(op, a, b, cplx))
    with open(os.path.join(HERE, "ref_digests.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests" % len(out))


if __name__ == "__main__":
    main()
