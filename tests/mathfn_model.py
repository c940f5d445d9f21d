"""What the tests of the real-valued function blocks share: the cases of tests/golden/mathfn.npz, the distance in units in the last
place, and a numpy model of the reference's float32 rsqrt (RSqrt.hpp), held to the recorded bits by test_mathfn_cpu.py."""
import os

import numpy as np

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mathfn.npz")
TYPES = ("float64", "float32")
TRIG = ("COS", "SIN", "TAN", "SEC", "CSC", "COT", "ACOS", "ASIN", "ATAN", "ASEC", "ACSC", "ACOT",
        "COSH", "SINH", "TANH", "SECH", "CSCH", "COTH", "ACOSH", "ASINH", "ATANH", "ASECH", "ACSCH", "ACOTH")
PLAIN = ("EXP", "EXP2", "EXP10", "EXPM1", "LOG", "LOG2", "LOG10", "LOG1P", "SQRT", "CBRT", "RSQRT", "SINC", "SIGMOID") + TRIG
PARAMS = {"POW": (2, 0.5, -1.5, 3), "EXPN": (2, 3, 0.5), "LOGN": (2, 3, 0.5), "NTH_ROOT": (2, 3, 4, 5, -3, 2.5)}
# (function, parameter or None), and the key of a case in the fixture
CASES = [(fn, None) for fn in PLAIN] + [(fn, p) for fn, ps in PARAMS.items() for p in ps]


def case_key(fn, p, tname):
    return "%s/%s" % (fn if p is None else "%s@%g" % (fn, p), tname)


def keys(a):
    """bit patterns as sign-magnitude integers: consecutive values of the type are consecutive keys, through zero and the subnormals"""
    a = np.ascontiguousarray(a)
    i = a.view(np.int64 if a.dtype == np.float64 else np.int32).astype(np.int64)
    mag = i & (0x7FFFFFFFFFFFFFFF if a.dtype == np.float64 else 0x7FFFFFFF)
    return np.where(i < 0, -mag, mag)


def ulp_distance(a, b):
    """|keys(a) - keys(b)|, taken in Python integers (the keys of float64 values of opposite sign differ by more than an int64 holds) and
    returned as float64: exact wherever it is small enough to be compared with a bar"""
    d = keys(a).astype(object) - keys(b).astype(object)
    return np.array([float(abs(v)) for v in d.reshape(-1)], dtype=np.float64).reshape(d.shape)


def rsqrt_f32(x):
    """RSqrt.hpp:13-25 in numpy: one integer subtraction on the bit pattern, then float32 products and one difference, each rounded"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        f2 = (np.uint32(0x5F1FFFF9) - (x.view(np.uint32) >> np.uint32(1))).view(np.float32)
        return (np.float32(0.703952253) * f2) * (np.float32(2.38924456) - (x * f2) * f2)
