"""/comms/envelope_detector restated in numpy: the magnitude the reference's getAbs<float> computes for each element type, the
gains its setters compute, and the float32 recurrence of EnvelopeDetector::work (tests/golden/make_envelope_golden.py records the
reference's own outputs, tests/test_envelope_cpu.py holds this restatement to them):

  floats        float(|x|); complex_float32: hypotf, complex_float64: hypot, then narrowed to float
  real ints     float(abs(x)) with abs in the promoted type: int8 -128 -> 128, int16 -32768 -> 32768, int32 / int64 MIN stays MIN
  complex ints  libstdc++'s generic __complex_abs in the element type T: s = T(max(abs(re), abs(im))); re /= s; im /= s (truncating);
                T(s * sqrt(re*re + im*im)) with the products wrapped, the sqrt in double and the final conversion as x86-64's
                cvttsd2si (out of range -> the minimum of int32 / int64; int8 / int16 truncate to int32, then wrap)
  step          e = (x > e) ? gA*e + oA*x : gR*e + oR*x, every product and sum rounded to float32
"""
import ctypes
import ctypes.util

import numpy as np

SCALARS = {"float64": np.float64, "float32": np.float32, "int64": np.int64, "int32": np.int32, "int16": np.int16, "int8": np.int8}
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def split(dtype):
    cplx = dtype.startswith("complex_")
    name = dtype[8:] if cplx else dtype
    if name not in SCALARS:
        raise ValueError("unsupported type " + dtype)
    return name, cplx


def gains(attack=None, release=None):
    """(gA, oA, gR, oR) as float32: std::exp(-1/t) in float (glibc's expf, as the reference and the port compute it), 1 - g.
    A time constant that was never set (None) leaves both of its gains 0."""
    out = []
    for t in (attack, release):
        if t is None:
            out += [np.float32(0), np.float32(0)]
            continue
        with np.errstate(divide="ignore"):
            arg = np.float32(-1) / np.float32(t)
        g = np.float32(_libm.expf(float(arg)))
        out += [g, np.float32(1) - g]
    return tuple(out)


def _wrap(v, bits):
    v = np.asarray(v, dtype=np.int64)
    if bits >= 64:
        return v
    m = np.int64(1) << np.int64(bits)
    h = np.int64(1) << np.int64(bits - 1)
    return ((v + h) & (m - 1)) - h


def _tdiv(a, b):
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        q = a // b
        r = a - q * b
    return q + ((r != 0) & ((a < 0) != (b < 0))).astype(np.int64)


def _cvtt(v, bits):
    """x86-64 cvttsd2si into `bits` (32 or 64): truncation, out of range or NaN -> the minimum"""
    lo, hi = (-2147483649.0, 2147483648.0) if bits == 32 else (-9223372036854775809.0, 9223372036854775808.0)
    ok = (v > lo) & (v < hi) if bits == 32 else (v >= -9223372036854775808.0) & (v < hi)
    with np.errstate(invalid="ignore"):
        t = np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0.0)
    out = t.astype(np.int64)
    return np.where(ok, out, np.int64(-(1 << (bits - 1))))


def _cplx_int_abs(re, im, bits):
    re = re.astype(np.int64)
    im = im.astype(np.int64)
    pb = max(bits, 32)                 # abs in the promoted type: int for int8 / int16 / int32, long for int64
    ar = _wrap(np.abs(re), pb)
    ai = _wrap(np.abs(im), pb)
    s = _wrap(np.maximum(ar, ai), bits)
    zero = s == 0
    s1 = np.where(zero, 1, s)
    x = _wrap(_tdiv(re, s1), bits)
    y = _wrap(_tdiv(im, s1), bits)
    with np.errstate(over="ignore"):
        m2 = _wrap(x * x + y * y, pb)  # int64 products wrap mod 2^64 in numpy as in the compiled header
    with np.errstate(invalid="ignore"):
        d = s.astype(np.float64) * np.sqrt(m2.astype(np.float64))
    v = _wrap(_cvtt(d, 32 if bits <= 32 else 64), bits)
    return np.where(zero, 0, v).astype(np.float32)


def magnitude(x, dtype):
    """getAbs<float>(x) of every element: (n,) real or (n, 2) complex pairs -> (n,) float32"""
    name, cplx = split(dtype)
    x = np.asarray(x)
    if not cplx:
        if name.startswith("float"):
            with np.errstate(over="ignore"):
                return np.abs(x).astype(np.float32)
        bits = np.dtype(SCALARS[name]).itemsize * 8
        return _wrap(np.abs(x.astype(np.int64)), max(bits, 32)).astype(np.float32)
    re, im = x[:, 0], x[:, 1]
    if name == "float32":
        with np.errstate(over="ignore", invalid="ignore"):
            r = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2).astype(np.float32)
        return np.where(np.isinf(re) | np.isinf(im), np.float32(np.inf), r)
    if name == "float64":
        with np.errstate(over="ignore"):
            return np.hypot(re, im).astype(np.float32)
    return _cplx_int_abs(re, im, np.dtype(SCALARS[name]).itemsize * 8)


def step_all(mag, prev, g):
    """one step of the recurrence for every (prev, mag) pair, float32 throughout"""
    gA, oA, gR, oR = g
    mag = np.asarray(mag, np.float32)
    prev = np.asarray(prev, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        up = gA * prev + oA * mag
        down = gR * prev + oR * mag
    return np.where(mag > prev, up, down).astype(np.float32)


def run(mag, g, state0=0.0):
    """the sequential loop: outputs and the final envelope"""
    mag = np.asarray(mag, np.float32)
    gA, oA, gR, oR = g
    e = np.float32(state0)
    out = np.empty(mag.shape[0], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i, xn in enumerate(mag):
            e = (gA * e + oA * xn) if xn > e else (gR * e + oR * xn)
            out[i] = e
    return out, e


def same(a, b):
    """bit-equal float32 arrays, any NaN equal to any NaN"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def check_steps(mag, out, state0, g):
    """out[i] == step(out[i-1], mag[i]) for every i (out[-1] := state0), checked at once: the index of the first output that
    breaks it, or -1"""
    out = np.asarray(out, np.float32)
    prev = np.concatenate([np.asarray([state0], np.float32), out[:-1]])
    want = step_all(mag, prev, g)
    ok = (want.view(np.uint32) == out.view(np.uint32)) | (np.isnan(want) & np.isnan(out))
    bad = np.nonzero(~ok)[0]
    return int(bad[0]) if bad.size else -1
