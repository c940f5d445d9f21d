"""Writes tests/golden/specfn.npz: inputs, what g++ and glibc give, and the correctly rounded truth for the special-function blocks
(math/Gamma.cpp, ErrorFunction.cpp, Beta.cpp, ModF.cpp of the reference).

A small driver of this project's own (DRIVER below) is compiled with the flags of make_mathfn_golden.py (g++ -std=c++17 -O3
-ffp-contract=off, no -march) and applies, element by element, the std:: call the reference's scalar loop applies.  Nothing compiled
is kept.  TRUTH is the same expression with every operation exact -- mpmath at 400 bits, rounded ONCE to the element type by
make_mathfn_golden.round_to.  For beta that is exp(ln|gamma(a)| + ln|gamma(b)| - ln|gamma(a + b)|) with a + b the exact sum, which is
|B(a, b)| where B is negative: the sign is lost in the expression, and the expression is the contract.  modf has no truth: it has
one right answer, which glibc gives.

Per function and type, "<FUNCTION>/<type>/...":
    ord    GAMMA, LNGAMMA, ERF, ERFC  (3, n)  rows: the ordinary inputs, `ref` (g++ and glibc), `cr` (the rounded truth)
           BETA                       (4, n)  rows: a, b, ref, cr
           MODF                       (3, n)  rows: x, the reference's integral part, the reference's fractional part
    e_ref  ()      the largest distance between ref and cr over the ordinary inputs, in units in the last place (not for MODF)
    large  BETA only  (4, n)  rows: a, b, ref, cr for a larger argument from 1024 (where csrc/specfn.hip leaves the term-by-term
           evaluation, both sides of that threshold included) to 1e12 against a smaller one in (0.01, 20), in either order; a draw
           of its own (seed 21), so the other groups do not depend on it
    spec   the same rows for the special inputs; cr only where ref is finite and not zero (NaN elsewhere: the bar there is
           NaN-ness resp. the value and its sign)
About 200 ordinary inputs per case on the domains of ordinary() below, seed 20.  THE CONDITIONS: the script fails if ref is more than
4 units from cr on an ordinary input of the four unary functions (move the domain, do not drop points), and if the reference's beta
is further from cr than specfn_model.beta_bound allows, in the units of the type it ran in.

    python tests/golden/make_specfn_golden.py [--out tests/golden/specfn.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import mpmath
import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_mathfn_golden import Driver, round_to, ulp_distance  # noqa: E402
import specfn_model as S  # noqa: E402

mp.prec = 400
N_ORD = 200
SEED = 20
TYPES = [("float64", np.float64), ("float32", np.float32)]

DRIVER = r"""
// driver <function> <float64|float32> <n> <in.bin> <out.bin>: BETA reads a[n] then b[n], MODF writes int[n] then frac[n]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <typename T>
static int run(const std::string &fn, size_t n, const char *fin, const char *fout)
{
    const size_t nin = fn == "BETA" ? 2 * n : n, nout = fn == "MODF" ? 2 * n : n;
    std::vector<T> x(nin), y(nout);
    FILE *f = std::fopen(fin, "rb");
    if (!f || std::fread(x.data(), sizeof(T), nin, f) != nin) return 2;
    std::fclose(f);
    for (size_t i = 0; i < n; i++) {
        const T v = x[i];
        if (fn == "GAMMA") y[i] = std::tgamma(v);
        else if (fn == "LNGAMMA") y[i] = std::lgamma(v);
        else if (fn == "ERF") y[i] = std::erf(v);
        else if (fn == "ERFC") y[i] = std::erfc(v);
        else if (fn == "BETA") y[i] = std::beta(v, x[n + i]);
        else if (fn == "MODF") y[n + i] = std::modf(v, &y[i]);
        else return 3;
    }
    f = std::fopen(fout, "wb");
    if (!f || std::fwrite(y.data(), sizeof(T), nout, f) != nout) return 4;
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 6) return 1;
    const std::string fn = argv[1], type = argv[2];
    const size_t n = std::strtoull(argv[3], nullptr, 10);
    return type == "float64" ? run<double>(fn, n, argv[4], argv[5]) : run<float>(fn, n, argv[4], argv[5]);
}
"""


class SpecDriver(Driver):
    """make_mathfn_golden.Driver's pattern with this script's driver string: compiled once into a temporary directory"""

    def __init__(self, wd):
        self.wd = wd
        src, self.exe = os.path.join(wd, "driver.cpp"), os.path.join(wd, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", src, "-o", self.exe])

    def run(self, fn, *xs):
        fin, fout = os.path.join(self.wd, "in.bin"), os.path.join(self.wd, "out.bin")
        np.concatenate(xs).tofile(fin)
        subprocess.check_call([self.exe, fn, xs[0].dtype.name, str(xs[0].size), fin, fout])
        return np.fromfile(fout, dtype=xs[0].dtype)


# ---------------------------------------------------------------- the expressions, exact
def ln_abs_gamma(x):
    return mpmath.loggamma(x) if x > 0 else mpmath.log(abs(mpmath.gamma(x)))


def truth(fn, x, y=None):
    if fn == "GAMMA":
        return mpmath.gamma(x)
    if fn == "LNGAMMA":
        return ln_abs_gamma(x)
    if fn == "ERF":
        return mpmath.erf(x)
    if fn == "ERFC":
        return mpmath.erfc(x)
    if fn == "BETA":
        return mpmath.exp(ln_abs_gamma(x) + ln_abs_gamma(y) - ln_abs_gamma(mpmath.fadd(x, y, exact=True)))
    raise KeyError(fn)


def rounded_truth(fn, dt, x, y=None):
    out = np.full(x.shape, np.nan, dtype=dt)
    for i in range(x.size):
        if np.isnan(x[i]) or (y is not None and np.isnan(y[i])):
            continue
        try:
            t = truth(fn, mpf(float(x[i])), None if y is None else mpf(float(y[i])))
        except (ZeroDivisionError, ValueError, OverflowError, TypeError):      # a pole: no finite truth
            continue
        if isinstance(t, mpmath.mpc) or not mpmath.isfinite(t):
            continue
        out[i] = round_to(t, dt)
    return out


# ---------------------------------------------------------------- inputs
def inside(v, lo, hi, dt):
    return np.clip(v.astype(dt), np.nextafter(dt(lo), dt(np.inf)), np.nextafter(dt(hi), dt(-np.inf)))


def ordinary(fn, dt, rng):
    if fn == "GAMMA":           # three quarters in (0.01, 20), one quarter in (-6, 0) clear of the integers (the poles)
        neg = -(rng.integers(0, 6, N_ORD // 4) + rng.uniform(0.1, 0.9, N_ORD // 4))
        return np.concatenate([inside(rng.uniform(0.01, 20, N_ORD - N_ORD // 4), 0.01, 20, dt), neg.astype(dt)])
    if fn == "LNGAMMA":         # positive, off the zeros at 1 and 2, where the function is ill-conditioned
        return np.concatenate([inside(rng.uniform(lo, hi, n), lo, hi, dt) for lo, hi, n in ((0.01, 0.75, 50), (1.25, 1.75, 30), (2.5, 20, N_ORD - 80))])
    if fn == "ERF":
        return inside(rng.uniform(-6, 6, N_ORD), -6, 6, dt)
    if fn == "ERFC":
        hi = 9 if dt == np.float32 else 25
        return inside(rng.uniform(-6, hi, N_ORD), -6, hi, dt)
    if fn == "BETA":
        return inside(rng.uniform(0.01, 20, N_ORD), 0.01, 20, dt), inside(rng.uniform(0.01, 20, N_ORD), 0.01, 20, dt)
    if fn == "MODF":            # a quarter spread over the decades
        m = rng.uniform(0, 2.0 ** 20, N_ORD)
        m[: N_ORD // 4] = np.exp(rng.uniform(np.log(1e-3), np.log(2.0 ** 20), N_ORD // 4))
        return inside(m, 0, 2.0 ** 20, dt) * rng.choice([-1.0, 1.0], N_ORD).astype(dt)
    raise KeyError(fn)


def large(dt):
    """beta's large arguments: the neighbourhood of 1024 on both sides, then the decades up to 1e12; the smaller argument in (0.01, 20)"""
    rng = np.random.default_rng(SEED + 1)
    edge = [np.nextafter(dt(1024), dt(0)), dt(1024), np.nextafter(dt(1024), dt(np.inf)), dt(1000), dt(1023.5), dt(1024.5), dt(1100)]
    x = np.concatenate([np.array(edge, dtype=dt), np.exp(rng.uniform(np.log(1024), np.log(1e12), 57)).astype(dt)])
    # (the smaller argument stays where the result, about gamma(y) x^-y, is a normal number of the type: y log10(x) at most 30 resp. 280)
    top = np.minimum(20, (30 if dt == np.float32 else 280) / np.log10(x.astype(np.float64)))
    y = (0.01 + rng.uniform(0, 1, x.size) * (top - 0.02)).astype(dt)
    y[:3] = dt(1)                          # B(x, 1) = 1 / x across the threshold
    swap = rng.integers(0, 2, x.size).astype(bool)
    return np.where(swap, y, x), np.where(swap, x, y)


def common(dt):
    fi = np.finfo(dt)
    tiny, big, sub = float(fi.tiny), float(fi.max), float(fi.smallest_subnormal)
    return [0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, big, -big, sub, -sub, 1.0, -1.0, 0.5, -0.5, 2.0, 3.0, -2.0, -3.0]


def special(fn, dt):
    f32 = dt == np.float32
    v = common(dt)
    if fn == "GAMMA":
        v += [-2.5, -3.75] + ([1e-30, 34.5, 35.0, 35.5, 36.0, -38.5, -41.5, -45.5, -50.5] if f32 else
                              [1e-300, 170.5, 171.5, 171.7, 172.0, -170.5, -177.5, -184.5, -190.5])
    if fn == "LNGAMMA":         # (not -2.5: |gamma(-2.5)| is 0.945, the logarithm next to a zero)
        v += [-1.5, -3.75, 100.5, -100.5, 1e10] + ([1e-30, -1e-30, 1e30, 4e36] if f32 else [1e-300, -1e-300, 1e300, 2.5e305])
    if fn in ("ERF", "ERFC"):
        v += [1e-30, -1e-30, 3.5, 4.5, -4.5, 6.0, -6.0, 9.0, 9.5, 10.5, 11.0] if f32 else [1e-300, -1e-300, 5.5, 6.5, -6.5, 26.0, 26.5, 27.0, 27.5, 28.0]
    if fn == "MODF":
        v += [2.5, -2.5, 3.75, -3.75, 1e10] + ([8388607.5, 8388607.0, 8388608.0, 8388609.0, -8388607.5, 16777216.0] if f32 else
                                                [4503599627370495.5, 4503599627370495.0, 4503599627370496.0, 4503599627370497.0, -4503599627370495.5,
                                                 9007199254740992.0])
    if fn == "BETA":            # the common list as a against b = 1, then swapped, plus two large arguments
        a = v + [1.0] * len(v) + [171.5, 1e10]
        b = [1.0] * len(v) + v + [1.0, 1.0]
        return np.array(a, dtype=dt), np.array(b, dtype=dt)
    return np.array(v, dtype=dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "specfn.npz"))
    a = ap.parse_args()
    rng = np.random.default_rng(SEED)
    arrays = {}
    with tempfile.TemporaryDirectory() as wd:
        drv = SpecDriver(wd)
        for fn in S.FUNCS:
            for tname, dt in TYPES:
                key = S.case_key(fn, tname)
                if fn == "MODF":
                    for part, x in (("ord", ordinary(fn, dt, rng)), ("spec", special(fn, dt))):
                        out = drv.run(fn, x)
                        arrays["%s/%s" % (key, part)] = np.stack([x, out[:x.size], out[x.size:]])
                    print("%-18s recorded" % key)
                    continue
                xs = ordinary(fn, dt, rng)
                xs = xs if isinstance(xs, tuple) else (xs,)
                ref = drv.run(fn, *xs)
                cr = rounded_truth(fn, dt, *xs)
                assert np.isfinite(ref).all() and np.isfinite(cr).all() and (cr != 0).all(), key
                d = ulp_distance(ref, cr)
                e_ref = int(max(d))
                worst = int(np.argmax(d))
                if fn == "BETA":
                    bound = S.beta_bounds(xs[0], xs[1], dt)
                    assert all(int(v) <= b for v, b in zip(d, bound)), "%s: the reference leaves its derived bound" % key
                    print("%-18s e_ref %d, derived bounds %d ... %d" % (key, e_ref, bound.min(), bound.max()))
                else:
                    assert e_ref <= 4, "%s: the reference is %d units from the truth at x = %r: move the domain" % (key, e_ref, xs[0][worst])
                    print("%-18s e_ref %d" % (key, e_ref))
                sx = special(fn, dt)
                sx = sx if isinstance(sx, tuple) else (sx,)
                sref = drv.run(fn, *sx)
                scr = rounded_truth(fn, dt, *sx)
                scr[~(np.isfinite(sref) & (sref != 0))] = np.nan
                arrays[key + "/ord"] = np.stack(list(xs) + [ref, cr])
                arrays[key + "/spec"] = np.stack(list(sx) + [sref, scr])
                arrays[key + "/e_ref"] = np.int64(e_ref)
                if fn == "BETA":
                    lx = large(dt)
                    arrays[key + "/large"] = np.stack(list(lx) + [drv.run(fn, *lx), rounded_truth(fn, dt, *lx)])
                    assert np.isfinite(arrays[key + "/large"]).all(), key
    np.savez_compressed(a.out, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (a.out, len(arrays), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
