"""Model, truth, bounds and inputs of /comms/signal_probe (utility/SignalProbe.cpp:123-163), shared by tests/test_probe_cpu.py and
tests/test_probe_gpu.py.

model(x, mode)   the reference's loop restated: every element converted to float64 resp. complex128, a SEQUENTIAL float64 accumulation
                 from +0.0 (numpy's add.accumulate adds in index order, one rounding per element, as `accumulator += v` does),
                 np.abs of the complex128 element for the modulus (the C library's hypot, as std::abs is), one division, np.sqrt.
truth(x, mode)   the exact value of the same expression over the converted doubles: the sum as a fractions.Fraction (the doubles are
                 taken apart into integer mantissas and summed as integers, exponent by exponent -- no rounding anywhere), the quotient
                 and the square root in mpmath at 400 bits, rounded once to double.
bound(...)       derived, never measured.  u = 2^-53, d = ceil(log2 N):
                   VALUE  0: a conversion to double is exact for every one of the twelve types (int64 rounds once, as the reference's does)
                   MEAN   per component (d + 2) u sum |x_n| / N: at most d additions round on the way of a term through the tree, one
                          division, and the second-order terms of (1 + u)^(d + 1) - 1
                   RMS    (d + 6) u truth: the modulus within 1 ulp (2u relative on its square) and the squaring (u) give 3u per term,
                          d u for the tree on non-negative terms, u for the division; the root halves that sum and adds u; the rest
                          covers the second-order terms and the truth's own rounding
                 The sequential model is only bound by about N u, hence model_bound().
"""
import functools
from fractions import Fraction

import mpmath
import numpy as np

TYPES = ["float64", "float32", "int64", "int32", "int16", "int8",
         "complex_float64", "complex_float32", "complex_int64", "complex_int32", "complex_int16", "complex_int8"]
MODES = ["VALUE", "RMS", "MEAN"]
U = 2.0 ** -53
BIG = (1 << 22) + 3
BIG_TYPES = ["float32", "int8", "complex_float64"]
FIXED_LENGTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257]


def is_complex(dtype):
    return dtype.startswith("complex_")


def scalar_of(dtype):
    return np.dtype(dtype[8:] if is_complex(dtype) else dtype)


def lengths(geometry):
    """the window lengths of the type matrix: the fixed ones and the seams of geometry() = (tile, slice, switch_over)"""
    tile, slc, switch = geometry
    out = list(FIXED_LENGTHS)
    for n in (tile - 1, tile, tile + 1, switch - 1, switch, switch + 1, 2 * slc + 3):
        if n not in out:
            out.append(n)
    return out


@functools.lru_cache(maxsize=None)
def make_input(dtype, n, seed=0):
    """n elements of `dtype`, (n,) or (n, 2) of the scalar type: magnitudes spread over many octaves; the float types with pairs of
    large values of opposite sign that cancel in the sum and small values between them; the integer types with their extremes (int64
    stays below 2^31 in magnitude, where its sums are exact in double).  Read-only: the tests share it."""
    sc = scalar_of(dtype)
    m = n * (2 if is_complex(dtype) else 1)
    rng = np.random.default_rng([seed, TYPES.index(dtype), n])
    if sc.kind == "f":
        span = 30 if sc == np.float32 else 60
        v = rng.uniform(1.0, 2.0, m) * np.exp2(rng.integers(-span, span + 1, m)) * rng.choice([-1.0, 1.0], m)
        v = v.astype(sc)
        pairs = min(m // 4, 6)
        if pairs:
            at = rng.permutation(m - 1)[:2 * pairs]          # (the last element stays what VALUE reads)
            big = (rng.uniform(1.0, 2.0, pairs) * 2.0 ** (span + 8)).astype(sc)
            v[at[0::2]] = big
            v[at[1::2]] = -big
    else:
        bits = 8 * sc.itemsize
        lo, hi = (-(2 ** 31 - 1), 2 ** 31 - 1) if sc == np.int64 else (np.iinfo(sc).min, np.iinfo(sc).max)
        v = rng.integers(lo, hi, m, endpoint=True, dtype=np.int64) >> rng.integers(0, min(bits, 32) - 1, m)
        v = v.astype(sc)
        if m >= 4:
            at = rng.permutation(m)[:4]
            v[at] = [hi, lo, hi, lo]
    v = v.reshape(n, 2) if is_complex(dtype) else v
    v.setflags(write=False)
    return v


def to_double(x):
    """the elements as the reference converts them: float64 of shape (n,), or complex128"""
    x = np.asarray(x)
    if x.ndim == 2:
        z = np.empty(x.shape[0], np.complex128)       # (component by component: signed zeros and infinities stay what they are)
        z.real = x[:, 0]
        z.imag = x[:, 1]
        return z
    return x.astype(np.float64)


def _seq_sum(terms):
    """accumulator = 0.0; for v in terms: accumulator += v"""
    return float(np.add.accumulate(np.concatenate([[0.0], terms]))[-1]) if len(terms) else 0.0


def model(x, mode):
    """(re, im) as the reference's work() leaves them in _value for one window"""
    z = to_double(x)
    n = len(z)
    cplx = np.iscomplexobj(z)
    with np.errstate(all="ignore"):
        if mode == "VALUE":
            return (float(z[-1].real), float(z[-1].imag)) if cplx else (float(z[-1]), 0.0)
        if mode == "RMS":
            v = np.abs(z)
            return float(np.sqrt(np.float64(_seq_sum(v * v)) / np.float64(n))), 0.0
        if cplx:
            return float(np.float64(_seq_sum(z.real)) / np.float64(n)), float(np.float64(_seq_sum(z.imag)) / np.float64(n))
        return float(np.float64(_seq_sum(z)) / np.float64(n)), 0.0


def _mantissas(v):
    """finite float64 v = m * 2^e with integer m (|m| < 2^53): (m as int64, e)"""
    f, e = np.frexp(v)
    return np.ldexp(f, 53).astype(np.int64), e.astype(np.int64) - 53


def _by_exponent(m, e):
    """the mantissas sorted by exponent: (m sorted, first index of every run of one exponent, that exponent)"""
    order = np.argsort(e.astype(np.int16), kind="stable")       # (a radix sort: the exponents of a double fit 16 bits)
    m, e = m[order], e[order]
    starts = np.flatnonzero(np.concatenate([[True], e[1:] != e[:-1]])) if len(e) else np.zeros(0, np.int64)
    return m, starts, e[starts]


def _assemble(parts, shifts, exps, base):
    """sum over the runs r of (sum over k of parts[k][r] << shifts[k]) * base^exps[r], in integers and Fractions"""
    total = Fraction(0)
    for r, ex in enumerate(exps):
        s = sum(int(p[r]) << sh for p, sh in zip(parts, shifts))
        total += Fraction(s) * Fraction(base) ** int(ex)
    return total


def exact_sum(v):
    """sum of finite float64 values, exactly: the mantissas in two halves, each run's sums far below 2^63"""
    m, e = _mantissas(np.asarray(v, np.float64))
    if not len(m):
        return Fraction(0)
    m, starts, exps = _by_exponent(m, e)
    parts = [np.add.reduceat(m >> 27, starts), np.add.reduceat(m & ((1 << 27) - 1), starts)]
    return _assemble(parts, [27, 0], exps, 2)


def exact_sum_squares(v):
    """sum of v^2 over finite float64 values, exactly: m = a 2^36 + b 2^18 + c, the five products summed apart (n < 2^24)"""
    m, e = _mantissas(np.asarray(v, np.float64))
    if not len(m):
        return Fraction(0)
    assert len(m) < 1 << 24
    m, starts, exps = _by_exponent(np.abs(m), e)
    k = (1 << 18) - 1
    a, b, c = m >> 36, (m >> 18) & k, m & k
    parts = [np.add.reduceat(t, starts) for t in (a * a, 2 * a * b, 2 * a * c + b * b, 2 * b * c, c * c)]
    return _assemble(parts, [72, 54, 36, 18, 0], exps, 4)


def _round_once(fr, root=False):
    """the Fraction fr (or its square root), rounded to double once"""
    if not root:
        return float(fr)                   # a Fraction converts correctly rounded
    with mpmath.workprec(400):
        return float(mpmath.sqrt(mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)))


def truth(x, mode):
    """(re, im) of the exact expression over the converted doubles, each rounded to double once"""
    z = to_double(x)
    n = len(z)
    cplx = np.iscomplexobj(z)
    if mode == "VALUE":
        return (float(z[-1].real), float(z[-1].imag)) if cplx else (float(z[-1]), 0.0)
    if mode == "RMS":
        s = exact_sum_squares(z.real) + exact_sum_squares(z.imag) if cplx else exact_sum_squares(z)
        return _round_once(s / n, root=True), 0.0
    if cplx:
        return _round_once(exact_sum(z.real) / n), _round_once(exact_sum(z.imag) / n)
    return _round_once(exact_sum(z) / n), 0.0


def _abs_sum(v):
    """sum |v| for a bound: numpy's pairwise sum of non-negative terms, within about 1e-15 of the exact one"""
    return float(np.sum(np.abs(v)))


def depth(n):
    return (n - 1).bit_length()            # ceil(log2 n)


def bound(x, mode, true):
    """(bound on re, bound on im) for the device's tree, from the derivation in the module docstring"""
    z = to_double(x)
    n, d = len(z), depth(len(z))
    if mode == "VALUE":
        return 0.0, 0.0
    if mode == "RMS":
        return (d + 6) * U * abs(true[0]), 0.0
    if np.iscomplexobj(z):
        return (d + 2) * U * _abs_sum(z.real) / n, (d + 2) * U * _abs_sum(z.imag) / n
    return (d + 2) * U * _abs_sum(z) / n, 0.0


def model_bound(x, mode, true):
    """what the sequential model is held to: max(the tree's bound, (N + 6) u scale)"""
    z = to_double(x)
    n = len(z)
    tree = bound(x, mode, true)
    if mode == "VALUE":
        return tree
    if mode == "RMS":
        return max(tree[0], (n + 6) * U * abs(true[0])), 0.0
    if np.iscomplexobj(z):
        return max(tree[0], (n + 6) * U * _abs_sum(z.real) / n), max(tree[1], (n + 6) * U * _abs_sum(z.imag) / n)
    return max(tree[0], (n + 6) * U * _abs_sum(z) / n), 0.0


def sum_is_exact(dtype, mode):
    """the cases in which every term and every partial sum is an integer below 2^53: any order of addition gives the same double"""
    sc = scalar_of(dtype)
    if sc.kind != "i":
        return False
    if mode == "MEAN":
        return True                        # int8, int16, int32 at every length used; int64 inputs stay below 2^31
    return mode == "RMS" and not is_complex(dtype) and sc.itemsize <= 2


@functools.lru_cache(maxsize=None)
def case(dtype, n, mode):
    """(truth, bound) of make_input(dtype, n) -- computed once per session"""
    x = make_input(dtype, n)
    t = truth(x, mode)
    return t, bound(x, mode, t)


def all_cases(geometry_of):
    """every (dtype, n) of the GPU suite's type matrix; geometry_of(dtype) -> (tile, slice, switch_over)"""
    out = []
    for dtype in TYPES:
        for n in lengths(geometry_of(dtype)):
            out.append((dtype, n))
        if dtype in BIG_TYPES:
            out.append((dtype, BIG))
    return out
