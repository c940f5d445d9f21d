"""What the tests of the special-function blocks share: the cases of tests/golden/specfn.npz, the distance in units in the last place
(mathfn_model's), a numpy model of modf, held to the recorded bits by test_specfn_cpu.py, and the per-input bound of beta.

THE BOUND OF BETA.  beta(a, b) is computed as exp(s), s = la + lb - lab, with la = lgamma(a), lb = lgamma(b), lab = lgamma(a + b).
Write u(v) for the unit in the last place of the value v in the type the expression runs in (u(0) = 0).  Each log-gamma is within
L units of its true value; half a unit more each is the allowance for the one operand that is itself rounded, a + b (its half unit
reaches lab through the digamma function, which stays below 3.7 on (0, 40); L is a ceiling several times what is measured):
(L + 1/2) u(la), (L + 1/2) u(lb), (L + 1/2) u(lab).  The sum la + lb is rounded, u(la + lb) / 2, and so is the difference,
u(la + lb - lab) / 2.  The absolute error E of s is at most the sum of these five terms, and an absolute error E of the exponent is a
relative error e^E - 1 = E + E^2 / 2 + ... of the result.  A relative error E is at most E * 2^p units in the last place of a type of
p significant bits (a unit is at least 2^-p of the value).  exp itself adds its own bar of 3 units, and 1 unit covers the second
order (E^2 / 2 * 2^p < 1 for every E below 2^-27, and the rounding of E * 2^p up):
    E   = (L + 1/2) (u(la) + u(lb) + u(lab)) + u(la + lb) / 2 + u(la + lb - lab) / 2
    bar = ceil(2^p E) + 3 + 1
with L = 16 (the ceiling DESIGN.md 21 holds the device library's lgamma to) and p = 53 for float64, 24 for float32 (where the
generator holds the REFERENCE's float32 expression to it).  The units are taken at the true values of la, lb and lab, rounded to the type.
The bound is wide -- thousands of units -- because that is what the expression costs: log-gamma values of some tens carry an
absolute error that the exponential turns into a relative one."""
import math
import os

import numpy as np

from mathfn_model import keys, ulp_distance  # noqa: F401  (shared with the tests)

GOLD_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "specfn.npz")
TYPES = ("float64", "float32")
UNARY = ("GAMMA", "LNGAMMA", "ERF", "ERFC")
FUNCS = UNARY + ("BETA", "MODF")
BETA_L = 16


def case_key(fn, tname):
    return "%s/%s" % (fn, tname)


def modf_model(x):
    """ModF.cpp:36 in numpy, the expression of csrc/specfn.hip: the truncation, and the exact difference with the sign of x; -> (int, frac)"""
    x = np.ascontiguousarray(x)
    with np.errstate(all="ignore"):
        ip = np.trunc(x)
        fp = np.where(np.isinf(x), np.copysign(x.dtype.type(0), x), np.copysign(x - ip, x))
    return ip, fp.astype(x.dtype)


def _unit(v, dt):
    v = dt(v)
    return 0.0 if v == 0 else float(np.spacing(np.abs(v)))


def beta_bound(la, lb, lab, dt):
    """the bar of the docstring for ONE input, in units in the last place of dt; la, lb, lab the true log-gamma values as floats"""
    p = 53 if dt == np.float64 else 24
    s1 = float(dt(la)) + float(dt(lb))
    e = (BETA_L + 0.5) * (_unit(la, dt) + _unit(lb, dt) + _unit(lab, dt)) + _unit(s1, dt) / 2 + _unit(s1 - float(dt(lab)), dt) / 2
    return math.ceil(2.0 ** p * e) + 3 + 1


def beta_bounds(a, b, dt):
    """beta_bound for arrays a, b off the poles: the true log-gamma values are taken from math.lgamma in double, within a few units of
    2^-53 of the truth, which moves a unit in the last place only where the value sits on a power of two"""
    out = np.empty(a.size, dtype=np.float64)
    for i, (u, v) in enumerate(zip(a.astype(np.float64).tolist(), b.astype(np.float64).tolist())):
        out[i] = beta_bound(math.lgamma(u), math.lgamma(v), math.lgamma(u + v), dt)
    return out
