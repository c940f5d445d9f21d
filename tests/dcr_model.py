"""/comms/dc_removal restated in numpy: the arithmetic the reference's compiled MovingAverage / DCRemoval perform, vectorised.

Per stage (filter/MovingAverage.hpp) the accumulator b1 is the running sum of the increments a0 = x[n] - x[n-D], and the
stage emits Type(b0 / D).  The running sum is a cumsum; integer wrap-around is a ring homomorphism, so wrapping the int64 cumsum
to the accumulator's width gives the accumulator bit for bit.  What narrows where (tests/golden/make_dcremoval_golden.py records
the reference's own outputs, tests/test_dcremoval_cpu.py holds this restatement to them):

  real int8   a0 exact (int), b1 wraps to int16, b0 = int16(b1) + a0 is NOT wrapped, y = int8(b0 / int16(D))
  real int16  a0 exact, b0 = b1 wrap to int32, y = int16(b0 / int32(D))
  real int32  a0 = int32(x - front) (the compiled header subtracts in 32 bits), b1 int64, y = int32(b1 / D)
  real int64  everything mod 2^64
  complex<T>  a0 = complex<T>(x - front): each component narrowed to T; b1 wraps to Acc; b0 / complex<Acc>(D, 0) is libstdc++'s
              generic integer division: re = Acc(re * D) / Acc(D * D), im = (im * D) / Acc(D * D) -- the imaginary numerator is
              an int for Acc = int16 and wraps to Acc otherwise -- each quotient narrowed to Acc, then to T
  floats      exact arithmetic (the reference's float running sum drifts: that drift is not reproduced): the window sum of the
              last D stage inputs in long double, divided by D, rounded to the element type
  out[n] = Type(x[n-D+1] - y_C[n])
"""
import numpy as np

SCALARS = {"float64": np.float64, "float32": np.float32, "int64": np.int64, "int32": np.int32, "int16": np.int16, "int8": np.int8}
ACC_BITS = {"int64": 64, "int32": 64, "int16": 32, "int8": 16}


def split(dtype):
    cplx = dtype.startswith("complex_")
    name = dtype[8:] if cplx else dtype
    if name not in SCALARS:
        raise ValueError("unsupported type " + dtype)
    return name, cplx


def wrap(v, bits):
    """two's-complement narrowing of int64 values to `bits`"""
    v = np.asarray(v, dtype=np.int64)
    if bits >= 64:
        return v
    m = np.int64(1) << np.int64(bits)
    h = np.int64(1) << np.int64(bits - 1)
    return ((v + h) & (m - 1)) - h


def tdiv(a, b):
    """C's truncating integer division, elementwise (b != 0)"""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    with np.errstate(over="ignore"):
        q = a // b
        r = a - q * b
    return q + ((r != 0) & ((a < 0) != (b < 0))).astype(np.int64)


def refused(dtype, D):
    """the divisor narrowed to the accumulator type is zero: the reference dies of SIGFPE, the port refuses the call"""
    name, cplx = split(dtype)
    if name not in ACC_BITS:
        return False
    m = 1 << ACC_BITS[name]
    d = D % m
    return (d * d % m if cplx else d) == 0


def _delayed(u, D):
    """u[k - D] with zeros before the stream"""
    out = np.zeros_like(u)
    if D < u.shape[0]:
        out[D:] = u[:u.shape[0] - D]
    return out


def _stage_int(u, D, name, cplx):
    """one MovingAverage stage over int64-held values of element type `name`; returns int64-held stage outputs"""
    tb = np.dtype(SCALARS[name]).itemsize * 8
    ab = ACC_BITS[name]
    ud = _delayed(u, D)
    with np.errstate(over="ignore"):
        if cplx or name in ("int32", "int64"):
            a = wrap(u - ud, tb)                 # complex<T> - complex<T>, int32 - int32: narrowed to T
        else:
            a = u - ud                           # promoted to int: exact
        b1 = wrap(np.cumsum(a, axis=0), ab)      # the accumulator after each step
        if not cplx:
            dd = wrap(D, ab)
            if name == "int8":
                prev = np.concatenate([np.zeros((1,), np.int64), b1[:-1]])
                b0 = prev + a                    # int16 + int16 -> int: not wrapped
            else:
                b0 = b1
            return wrap(tdiv(b0, dd), tb)
        dd = int(wrap(D, ab))
        nrm = wrap(dd * dd, ab)
        re = wrap(b1[:, 0] * dd, ab)
        im = b1[:, 1] * dd if ab == 16 else wrap(b1[:, 1] * dd, ab)
        y = np.stack([wrap(tdiv(re, nrm), ab), wrap(tdiv(im, nrm), ab)], axis=1)
        return wrap(y, tb)


def _stage_float(u, D, np_t):
    """exact-arithmetic stage: window sum of the last D inputs in long double / D, rounded to the element type"""
    p = np.cumsum(u.astype(np.longdouble), axis=0)
    s = p - _delayed(p, D)
    return (s / np.longdouble(D)).astype(np_t)


def restate(x, dtype, D, C):
    """out for a stream x fed after a reset (complex streams as (n, 2) arrays of the scalar type)"""
    name, cplx = split(dtype)
    np_t = SCALARS[name]
    x = np.asarray(x, dtype=np_t)
    if name in ACC_BITS:
        if refused(dtype, D):
            raise ZeroDivisionError("divisor narrowed to the accumulator is zero")
        u0 = x.astype(np.int64)
        y = u0
        for _ in range(C):
            y = _stage_int(y, D, name, cplx)
        front = _delayed(u0, D - 1)
        with np.errstate(over="ignore"):
            return wrap(front - y, np.dtype(np_t).itemsize * 8).astype(np_t)
    y = x
    for _ in range(C):
        y = _stage_float(y, D, np_t)
    return (_delayed(x, D - 1) - y).astype(np_t)
