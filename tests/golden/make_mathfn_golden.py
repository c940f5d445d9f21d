"""Writes tests/golden/mathfn.npz: inputs, what g++ and glibc give, and the correctly rounded truth for the real-valued function
blocks (math/Exp.cpp, Log.cpp, Pow.cpp, Root.cpp, RSqrt.cpp, Sinc.cpp, Sigmoid.cpp, Trigonometric.cpp of the reference).

A small driver of this project's own (DRIVER below) is compiled with the oracle's flags (g++ -O3 -ffp-contract=off, no -march) and
applies, element by element, the std:: call or the expression the reference's scalar loop applies.  Nothing compiled is kept.

TRUTH is the same expression with every operation exact: mpmath at 400 bits, rounded ONCE to the element type, to nearest, ties to
even, overflow to infinity and gradual underflow included -- the choice between the neighbouring values of the type is made by exact
comparison (round_to), never by float() followed by a narrowing, which rounds twice.  Parameters enter as the values the expression
sees: a base or an exponent as a value of the element type, the exponent of nth_root as the double 1.0 / root, the 1e-6 of sinc as
the double it is.  The float32 rsqrt of the reference is an approximation by construction (RSqrt.hpp); its truth is that polynomial
of the bit-shifted seed with exact arithmetic, so e_ref measures its four float32 roundings, not its distance from 1 / sqrt.

Per function (and parameter value) and type, "<case>/<type>/...":
    ord    (3, n)  rows: the ordinary inputs, `ref` (g++ and glibc), `cr` (the rounded truth)
    e_ref  ()      the largest distance between ref and cr over the ordinary inputs, in units in the last place: the difference of
                   the bit patterns read as sign-magnitude integers, uniform through the subnormals
    spec   (3, m)  rows: the special inputs, ref, cr -- cr only where ref is finite and not zero (NaN elsewhere: the bar there is
                   NaN-ness resp. the value and its sign)
    p      ()      the parameter, for expN, logN, pow and nth_root
About 200 ordinary inputs per case on the DOMAINS below, seed 20.  THE CONDITION: the script fails if ref is more than 4 units from
cr on an ordinary input (the formula is then ill-conditioned there or overflows inside: move the domain, do not drop points), and,
for the f(1 / x) operations, if the condition number |y f'(y) / f(y)| at y = 1 / x exceeds 2 anywhere on the domain.

Special inputs: +-0, +-inf, NaN, the smallest and the largest normal numbers, subnormals, +-1, and per function the edges of its
domain (log(-1), acos(1.5), atanh(+-1), acosh(1) ...), the overflow and underflow thresholds of exp, exp2 and sinh, the trigonometric
arguments 1e6 and 1e22, the neighbourhood of sinc's 1e-6, negative numbers for the roots.  Left out on purpose: inputs where the
reference's float32 expression overflows INSIDE although the exact expression does not -- sigmoid(-100) and csch(90), where it
returns 0 for a small true value, and the float32 subnormals below 2^-128 for the six f(1 / x) operations, whose reciprocal is an
infinity in float32 (asech and acsch then return an infinity for a true value near 100); a subnormal above 2^-128 stays in those
groups.  DESIGN.md 20 lists that as the one known departure.

    python tests/golden/make_mathfn_golden.py [--out tests/golden/mathfn.npz]
"""
import argparse
import math
import os
import subprocess
import tempfile

import mpmath
import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
mp.prec = 400
N_ORD = 200
SEED = 20
TYPES = [("float64", np.float64), ("float32", np.float32)]

TRIG = ["COS", "SIN", "TAN", "SEC", "CSC", "COT", "ACOS", "ASIN", "ATAN", "ASEC", "ACSC", "ACOT",
        "COSH", "SINH", "TANH", "SECH", "CSCH", "COTH", "ACOSH", "ASINH", "ATANH", "ASECH", "ACSCH", "ACOTH"]
PLAIN = ["EXP", "EXP2", "EXP10", "EXPM1", "LOG", "LOG2", "LOG10", "LOG1P", "SQRT", "CBRT", "RSQRT", "SINC", "SIGMOID"] + TRIG
PARAMS = {"POW": [2, 0.5, -1.5, 3], "EXPN": [2, 3, 0.5], "LOGN": [2, 3, 0.5], "NTH_ROOT": [2, 3, 4, 5, -3, 2.5]}
INVERSE_RECIPROCAL = {"ASEC": mpmath.acos, "ACSC": mpmath.asin, "ACOT": mpmath.atan, "ASECH": mpmath.acosh, "ACSCH": mpmath.asinh, "ACOTH": mpmath.atanh}

# ordinary inputs: |x| in [lo, hi], both signs where `signed`
DOMAINS = {
    "EXP": (0, 20, True), "EXP2": (0, 20, True), "EXP10": (0, 20, True), "EXPM1": (0, 20, True),
    "LOG": (1e-3, 20, False), "LOG2": (1e-3, 20, False), "LOG10": (1e-3, 20, False), "LOG1P": (-0.9, 20, None),
    "SQRT": (0, 20, False), "CBRT": (0, 20, True), "RSQRT": (1e-3, 20, False), "SINC": (1e-3, 20, True), "SIGMOID": (0, 20, True),
    "COS": (0, 20, True), "SIN": (0, 20, True), "TAN": (0, 20, True), "SEC": (0, 20, True), "CSC": (1e-3, 20, True), "COT": (1e-3, 20, True),
    "ACOS": (0, 1, True), "ASIN": (0, 1, True), "ATAN": (0, 20, True),
    "ASEC": (1.4, 20, True), "ACSC": (1.4, 20, True), "ACOT": (0.05, 20, True),          # (asec, acsc: acos and asin next to 1 are ill-conditioned)
    "COSH": (0, 20, True), "SINH": (0, 20, True), "TANH": (0, 20, True), "SECH": (0, 20, True), "CSCH": (1e-3, 20, True), "COTH": (1e-3, 20, True),
    "ACOSH": (1, 20, False), "ASINH": (0, 20, True), "ATANH": (0, 0.99, True),
    "ASECH": (0.05, 0.7, False), "ACSCH": (0.05, 20, True), "ACOTH": (1.3, 20, True),    # (asech, acoth: acosh and atanh next to 1)
    "POW": (1e-3, 20, False), "EXPN": (0, 20, True), "LOGN": (1e-3, 20, False), "NTH_ROOT": (1e-3, 20, False),
}

DRIVER = r"""
// driver <function> <float64|float32> <n> <parameter> <in.bin> <out.bin>: out[i] = the function's expression of in[i]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static float fast_rsqrt(float f)
{
    uint32_t u;
    float f2;
    std::memcpy(&u, &f, 4);
    u = 0x5F1FFFF9ul - (u >> 1);
    std::memcpy(&f2, &u, 4);
    return 0.703952253f * f2 * (2.38924456f - f * f2 * f2);
}
static float rsqrt1(float x) { return fast_rsqrt(x); }
static double rsqrt1(double x) { return 1.0 / std::sqrt(x); }
static float exp10_1(float x) { return ::exp10f(x); }
static double exp10_1(double x) { return ::exp10(x); }

template <typename T>
static int run(const std::string &fn, T p, size_t n, const char *fin, const char *fout)
{
    std::vector<T> x(n), y(n);
    FILE *f = std::fopen(fin, "rb");
    if (!f || std::fread(x.data(), sizeof(T), n, f) != n) return 2;
    std::fclose(f);
    const bool odd = std::fmod(p, T(2.0)) == 1;
    for (size_t i = 0; i < n; i++) {
        const T v = x[i];
        T r;
        if (fn == "EXP") r = std::exp(v);
        else if (fn == "EXP2") r = std::exp2(v);
        else if (fn == "EXP10") r = exp10_1(v);
        else if (fn == "EXPM1") r = std::expm1(v);
        else if (fn == "LOG") r = std::log(v);
        else if (fn == "LOG2") r = std::log2(v);
        else if (fn == "LOG10") r = std::log10(v);
        else if (fn == "LOG1P") r = std::log1p(v);
        else if (fn == "SQRT") r = T(std::sqrt(v));
        else if (fn == "CBRT") r = T(std::cbrt(v));
        else if (fn == "RSQRT") r = rsqrt1(v);
        else if (fn == "SINC") r = (std::abs(v) < 1e-6) ? 1 : (std::sin(v) / v);
        else if (fn == "SIGMOID") r = T(1.0) / (T(1.0) + std::exp(-v));
        else if (fn == "COS") r = std::cos(v);
        else if (fn == "SIN") r = std::sin(v);
        else if (fn == "TAN") r = std::tan(v);
        else if (fn == "SEC") r = T(1.0) / std::cos(v);
        else if (fn == "CSC") r = T(1.0) / std::sin(v);
        else if (fn == "COT") r = T(1.0) / std::tan(v);
        else if (fn == "ACOS") r = std::acos(v);
        else if (fn == "ASIN") r = std::asin(v);
        else if (fn == "ATAN") r = std::atan(v);
        else if (fn == "ASEC") r = std::acos(T(1.0) / v);
        else if (fn == "ACSC") r = std::asin(T(1.0) / v);
        else if (fn == "ACOT") r = std::atan(T(1.0) / v);
        else if (fn == "COSH") r = std::cosh(v);
        else if (fn == "SINH") r = std::sinh(v);
        else if (fn == "TANH") r = std::tanh(v);
        else if (fn == "SECH") r = T(1.0) / std::cosh(v);
        else if (fn == "CSCH") r = T(1.0) / std::sinh(v);
        else if (fn == "COTH") r = T(1.0) / std::tanh(v);
        else if (fn == "ACOSH") r = std::acosh(v);
        else if (fn == "ASINH") r = std::asinh(v);
        else if (fn == "ATANH") r = std::atanh(v);
        else if (fn == "ASECH") r = std::acosh(T(1.0) / v);
        else if (fn == "ACSCH") r = std::asinh(T(1.0) / v);
        else if (fn == "ACOTH") r = std::atanh(T(1.0) / v);
        else if (fn == "EXPN") r = std::pow(p, v);
        else if (fn == "LOGN") r = std::log(v) / std::log(p);
        else if (fn == "POW") r = T(std::pow(v, p));
        else if (fn == "NTH_ROOT") {
            if (odd) {
                const T s = T((v < 0) ? -1 : 1);
                r = T(std::pow(v * s, 1.0 / p) * s);
            } else
                r = T(std::pow(v, 1.0 / p));
        } else
            return 3;
        y[i] = r;
    }
    f = std::fopen(fout, "wb");
    if (!f || std::fwrite(y.data(), sizeof(T), n, f) != n) return 4;
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 7) return 1;
    const std::string fn = argv[1], type = argv[2];
    const size_t n = std::strtoull(argv[3], nullptr, 10);
    const double p = std::strtod(argv[4], nullptr);      // (a hexadecimal float: exact)
    return type == "float64" ? run<double>(fn, p, n, argv[5], argv[6]) : run<float>(fn, (float)p, n, argv[5], argv[6]);
}
"""


class Driver:
    def __init__(self, wd):
        self.wd = wd
        src, self.exe = os.path.join(wd, "driver.cpp"), os.path.join(wd, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", src, "-o", self.exe])

    def run(self, fn, x, p):
        fin, fout = os.path.join(self.wd, "in.bin"), os.path.join(self.wd, "out.bin")
        x.tofile(fin)
        subprocess.check_call([self.exe, fn, x.dtype.name, str(x.size), float(p).hex(), fin, fout])
        return np.fromfile(fout, dtype=x.dtype)


# ---------------------------------------------------------------- distances and the one rounding
def keys(a):
    """bit patterns as sign-magnitude integers: consecutive values of the type are consecutive keys, through zero and the subnormals"""
    a = np.ascontiguousarray(a)
    i = a.view(np.int64 if a.dtype == np.float64 else np.int32).astype(np.int64)
    mag = i & (0x7FFFFFFFFFFFFFFF if a.dtype == np.float64 else 0x7FFFFFFF)
    return np.where(i < 0, -mag, mag)


def ulp_distance(a, b):
    d = keys(a).astype(object) - keys(b).astype(object)        # (Python integers: no overflow between -max and +max)
    return np.array([abs(v) for v in d], dtype=object)


def round_to(v, dt):
    """the value of type dt nearest to the mpf v, ties to even, overflow to infinity: neighbours compared exactly"""
    fi = np.finfo(dt)
    if v == 0:
        return dt(0.0)
    sign, a = (-1 if v < 0 else 1), abs(v)
    big = mpf(float(fi.max))
    if a >= big + mpf(2) ** (fi.maxexp - fi.nmant - 2):       # at or beyond the midpoint of max and 2^maxexp: the tie goes to the even 2^maxexp
        return dt(sign * np.inf)
    with np.errstate(over="ignore", under="ignore"):
        c = dt(min(float(a), float(fi.max)))                   # a first guess, possibly rounded twice: one of the three below is right
    cands = {float(c), float(np.nextafter(c, dt(0))), float(min(np.nextafter(c, dt(np.inf)), fi.max))}
    best = None
    for cand in cands:
        err = abs(mpf(cand) - a)
        odd = int(keys(np.array([cand], dtype=dt))[0]) & 1
        if best is None or (err, odd) < best[0]:
            best = ((err, odd), cand)
    return dt(sign * best[1])


# ---------------------------------------------------------------- the expressions, exact
def truth(fn, x, p, dt, raw):
    """the expression of fn at the mpf x (raw: the same input as a value of the type, which still has the sign of a zero); p the
    parameter as the expression sees it"""
    m = mpmath
    if fn in INVERSE_RECIPROCAL:
        if x == 0:              # 1 / +-0 is the infinity of that sign
            return INVERSE_RECIPROCAL[fn](mpf("-inf") if np.signbit(raw) else mpf("inf"))
        return INVERSE_RECIPROCAL[fn](1 / x)
    simple = {"EXP": m.exp, "EXPM1": m.expm1, "LOG": m.log, "LOG10": m.log10, "LOG1P": m.log1p, "SQRT": m.sqrt, "CBRT": m.cbrt,
              "COS": m.cos, "SIN": m.sin, "TAN": m.tan, "SEC": m.sec, "CSC": m.csc, "COT": m.cot, "ACOS": m.acos, "ASIN": m.asin, "ATAN": m.atan,
              "COSH": m.cosh, "SINH": m.sinh, "TANH": m.tanh, "SECH": m.sech, "CSCH": m.csch, "COTH": m.coth,
              "ACOSH": m.acosh, "ASINH": m.asinh, "ATANH": m.atanh}
    if fn == "CBRT":
        return -m.cbrt(-x) if x < 0 else m.cbrt(x)
    if fn in simple:
        return simple[fn](x)
    if fn == "EXP2":
        return mpf(2) ** x
    if fn == "EXP10":
        return mpf(10) ** x
    if fn == "LOG2":
        return m.log(x, 2)
    if fn == "SINC":
        return mpf(1) if abs(x) < mpf(1e-6) else m.sin(x) / x
    if fn == "SIGMOID":
        return 1 / (1 + m.exp(-x))
    if fn == "RSQRT":
        if dt == np.float64:
            return 1 / m.sqrt(x)
        xf = np.array([raw], np.float32)
        f2 = (np.uint32(0x5F1FFFF9) - (xf.view(np.uint32) >> np.uint32(1))).view(np.float32)
        if not np.isfinite(f2[0]):
            return None
        f2 = mpf(float(f2[0]))
        return mpf(float(np.float32(0.703952253))) * f2 * (mpf(float(np.float32(2.38924456))) - x * f2 * f2)
    if fn == "EXPN":
        return p ** x
    if fn == "LOGN":
        return m.log(x) / m.log(p)
    if fn == "POW":
        return x ** p
    if fn == "NTH_ROOT":
        inv = mpf(1.0 / float(p))            # the double division of the expression
        if math.fmod(float(p), 2.0) == 1:
            f = -1 if x < 0 else 1
            return (x * f) ** inv * f
        return x ** inv
    raise KeyError(fn)


def rounded_truth(fn, x, p, dt):
    out = np.full(x.shape, np.nan, dtype=dt)
    pm = None if p is None else mpf(float(dt(p)))
    for i, v in enumerate(x):
        try:
            t = truth(fn, mpf(float(v)), pm, dt, v)
        except (ZeroDivisionError, ValueError, OverflowError):      # outside the expression's domain: no finite truth
            continue
        if t is None or isinstance(t, mpmath.mpc) or not mpmath.isfinite(t):
            continue
        out[i] = round_to(t, dt)
    return out


# ---------------------------------------------------------------- inputs
def ordinary(fn, p, dt, rng):
    lo, hi, signed = DOMAINS[fn]
    if signed is None:          # a plain interval
        return np.clip(rng.uniform(lo, hi, N_ORD).astype(dt), dt(lo), dt(hi))
    m = rng.uniform(lo, hi, N_ORD)
    m[: N_ORD // 4] = np.exp(rng.uniform(np.log(max(lo, 1e-3)), np.log(hi), N_ORD // 4))         # a quarter spread over the decades
    m = np.clip(m.astype(dt), np.nextafter(dt(lo), dt(np.inf)), np.nextafter(dt(hi), dt(0)))     # (strictly inside, in the type)
    if fn == "NTH_ROOT" and p in (3, 5):
        signed = True           # the mirrored path: a negative input has a root
    return m * rng.choice([-1.0, 1.0], N_ORD).astype(dt) if signed else m


def special(fn, dt):
    fi = np.finfo(dt)
    sub = float(fi.smallest_subnormal)
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, float(fi.tiny), -float(fi.tiny), float(fi.max), -float(fi.max), sub, -sub, sub * 1000, float(fi.tiny) / 2,
         1.0, -1.0, 0.5, 2.0]
    f32 = dt == np.float32
    if fn in ("LOG", "LOG2", "LOG10", "LOGN"):
        v += [-2.0, 10.0, 1e-30]
    if fn == "LOG1P":
        v += [-1.0, -2.0, -0.999999, 1e-20]
    if fn in ("ACOS", "ASIN"):
        v += [1.5, -1.5, 0.999999, -0.999999]
    if fn == "ATANH":
        v += [1.5, -1.5, 0.999999]
    if fn in ("ACOSH",):
        v += [0.5, 1.000001, 1e30]
    if fn == "EXP":
        v += [88.0, 88.5, 89.0, -87.0, -88.0, -103.0, -104.5] if f32 else [709.0, 709.5, 710.0, -708.0, -709.0, -745.0, -746.0]
    if fn == "EXP2":
        v += [127.0, 127.5, 128.0, -126.0, -127.0, -149.0, -150.5] if f32 else [1023.0, 1023.5, 1024.0, -1022.0, -1023.0, -1074.0, -1075.5]
    if fn == "SINH":
        v += [89.0, 89.5, 90.0, -89.0, -90.0] if f32 else [710.0, 710.4, 711.0, -710.0, -711.0]
    if fn in ("EXP10",):
        v += [38.0, 38.6, -37.5, -46.0] if f32 else [308.0, 308.3, -307.5, -324.5]
    if fn in ("COS", "SIN", "TAN", "SEC", "CSC", "COT", "SINC"):
        v += [1e6, -1e6, 1e22, -1e22]
    if fn == "SINC":
        v += [1e-7, -1e-7, 9.9e-7, 1.1e-6, -1.1e-6]
    if fn in ("SQRT", "RSQRT", "CBRT", "NTH_ROOT", "POW"):
        v += [-4.0, 4.0, -8.0, 8.0, 27.0, -27.0, 1e-30, 1e30]
    v = np.array(v, dtype=dt)
    if f32 and fn in INVERSE_RECIPROCAL:            # 1 / x overflows in float32 and not in the exact expression: the known departure
        with np.errstate(over="ignore", divide="ignore"):
            v = v[~(np.isinf(dt(1) / v) & (v != 0))]
    return v


def condition_check(fn, x):
    f = INVERSE_RECIPROCAL[fn]
    worst = 0
    for v in x:
        y = 1 / mpf(float(v))
        worst = max(worst, abs(y * mpmath.diff(f, y) / f(y)))
    assert worst <= 2, "%s: the condition number of the inverse function at 1 / x reaches %s on the domain" % (fn, mpmath.nstr(worst, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "mathfn.npz"))
    a = ap.parse_args()
    rng = np.random.default_rng(SEED)
    arrays = {}
    cases = [(fn, None) for fn in PLAIN] + [(fn, p) for fn, ps in PARAMS.items() for p in ps]
    with tempfile.TemporaryDirectory() as wd:
        drv = Driver(wd)
        for fn, p in cases:
            for tname, dt in TYPES:
                key = "%s/%s" % (fn if p is None else "%s@%g" % (fn, p), tname)
                x = ordinary(fn, p, dt, rng)
                if fn in INVERSE_RECIPROCAL:
                    condition_check(fn, x)
                ref = drv.run(fn, x, 0 if p is None else p)
                cr = rounded_truth(fn, x, p, dt)
                assert np.isfinite(ref).all() and np.isfinite(cr).all(), key
                d = ulp_distance(ref, cr)
                e_ref = int(max(d))
                assert e_ref <= 4, "%s: the reference is %d units from the truth at x = %r: move the domain" % (key, e_ref, x[int(np.argmax(d))])
                sx = special(fn, dt)
                sref = drv.run(fn, sx, 0 if p is None else p)
                scr = rounded_truth(fn, sx, p, dt)
                scr[~(np.isfinite(sref) & (sref != 0))] = np.nan
                arrays[key + "/ord"] = np.stack([x, ref, cr])
                arrays[key + "/spec"] = np.stack([sx, sref, scr])
                arrays[key + "/e_ref"] = np.int64(e_ref)
                if p is not None:
                    arrays[key + "/p"] = dt(p)
                print("%-24s e_ref %d" % (key, e_ref))
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (a.out, len(arrays), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
