"""Seeded inputs of the CPU checks against the compiled reference (oracle/_ref), shared by those tests and by make_ref_digests.py.

make_ref_digests.py stores a SHA-256 digest of what the compiled reference computes on each case in ref_digests.json, so that the
checks stay bit-exact where oracle/_ref is not built (it needs the reference sources); where it is built, the tests compare with it
directly as well.  A digest covers dtype, shape and every byte of the output.
"""
import hashlib

import numpy as np

FFT_SIZES = [1, 2, 6, 7, 12, 25, 27, 30, 32, 49, 60, 121, 128, 360, 1000, 2048]


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s %r " % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def fft_cases(n):
    """-> (key, frames, inverse): three frames of n bins in float32, float64 and int16, forward and inverse"""
    rng = np.random.default_rng(n)
    for inv in (False, True):
        yield "fft/%d/%d/f32" % (n, inv), rng.uniform(-1, 1, (3 * n, 2)).astype(np.float32), inv
        yield "fft/%d/%d/f64" % (n, inv), rng.uniform(-1, 1, (3 * n, 2)), inv
        yield "fft/%d/%d/i16" % (n, inv), rng.integers(-32768, 32768, (3 * n, 2)).astype(np.int16), inv


def atan2_pairs():
    """-> [(y, x)]: 50,000 random int16 pairs, then the grid near the axes and diagonals in both orders"""
    rng = np.random.default_rng(0)
    ys, xs = rng.integers(-32768, 32768, 50000), rng.integers(-32768, 32768, 50000)
    pairs = [(int(y), int(x)) for y, x in zip(ys, xs)]
    for v in range(-300, 300):
        for w in (-32768, -1, 0, 1, 32767, v, -v):
            pairs += [(v, w), (w, v)]
    return pairs


def arith_cases(o):
    """-> (key, op, a, b, is_complex) over every element type of the oracle `o`, real and complex: ADD / SUB / MUL on wide random
    operands, DIV on operands whose integer divisors are small and non-zero"""
    rng = np.random.default_rng(5)
    for code, dt in o.NP_SCALAR.items():
        for cplx in (False, True):
            shape = (5000, 2) if cplx else (5000,)
            if np.issubdtype(dt, np.floating):
                a = (rng.standard_normal(shape) * 100).astype(dt)
                b = (rng.standard_normal(shape) * 10).astype(dt)
                ad, bd = a, b
            else:
                info = np.iinfo(dt)
                a = rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True)
                b = rng.integers(info.min, info.max, size=shape, dtype=dt, endpoint=True)
                small = rng.integers(-9 if info.min < 0 else 1, 10, size=shape)
                bd = np.where(small == 0, 3, small).astype(dt)
                ad = (a // 4).astype(dt)
            for op, name in ((o.ADD, "ADD"), (o.SUB, "SUB"), (o.MUL, "MUL")):
                yield "arith/%s/%d/%s" % (np.dtype(dt).name, cplx, name), op, a, b, cplx
            yield "arith/%s/%d/DIV" % (np.dtype(dt).name, cplx), o.DIV, ad, bd, cplx
