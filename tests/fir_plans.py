"""The table of FIR plans that tests/test_fir_plans_gpu.py, tests/test_fir_truth_cpu.py and tests/test_fir_truth_gpu.py share.

The planner (pothoscomms_amd/csrc/fir_plan.hpp) picks one of about twenty plans from the handle's settings, and the algorithm AUTO
stands for.  PLANS holds at least one row for each plan and each answer of AUTO, and a row on either side of every bound that
decides a plan.  Each row names the last_algo and the last_plan its call must report; _taps and _stream give the row's own
seeded taps and input.  (A plain module: nothing here needs a GPU.)
"""
import collections
import zlib

import numpy as np

from tests.util import TOL

Row = collections.namedtuple("Row", "name dtype taps ntaps L M algo want bar tapgen plan")


def R(name, dtype, taps, ntaps, L=1, M=1, algo="AUTO", want="OLS_FFT", bar=None, tapgen="normal", plan=None):
    return Row(name, dtype, taps, ntaps, L, M, algo, want, bar, tapgen, plan)


# plan: the name (pothoscomms_amd._lib.FIR_PLANS) that FirFilter.last_plan must report after the row's call: the plan
# fir_resolve (fir_plan.hpp) gave the call, where last_algo says only which of three algorithms
# bar: None = the default of the type (integers and EXACT bit for bit, float64 1e-13, float32 TOL); a number = the float32 bar of
# that plan's own parity test (tests/test_parity_gpu.py, tests/test_fuzz_gpu.py)
PLANS = [
    # -- complex_float32, M = L = 1 --
    R("cf32 direct tile K=1 (AUTO: the unit tap stays exact)", "complex_float32", "COMPLEX", 1, want="DIRECT", plan="CF32_DIRECT_TILE"),
    R("cf32 direct tile K=255 DIRECT", "complex_float32", "COMPLEX", 255, algo="DIRECT", want="DIRECT", plan="CF32_DIRECT_TILE"),
    R("cf32 4096-sample K=1 OLS_FFT", "complex_float32", "COMPLEX", 1, algo="OLS_FFT", plan="CF32_OLS4096"),
    R("cf32 4096-sample K=255", "complex_float32", "COMPLEX", 255, plan="CF32_OLS4096"),
    R("cf32 4096-sample K=2049 real taps", "complex_float32", "REAL", 2049, plan="CF32_OLS4096"),
    R("cf32 4096-sample K=2049", "complex_float32", "COMPLEX", 2049, plan="CF32_OLS4096"),
    R("cf32 partitioned K=2050", "complex_float32", "COMPLEX", 2050, plan="CF32_UPOLS"),
    R("cf32 partitioned K=4097", "complex_float32", "COMPLEX", 4097, plan="CF32_UPOLS"),
    R("cf32 partitioned K=8193", "complex_float32", "COMPLEX", 8193, plan="CF32_UPOLS"),
    R("cf32 sliding EXACT K=8194 (beyond every frequency-domain plan)", "complex_float32", "COMPLEX", 8194, want="EXACT", plan="SLIDE"),
    # -- complex_float32 decimating: the folded spectrum (CF32_DECIM) for M = 2 and 4 / 8 / 16-fold, the strided polyphase kernel else --
    R("cf32 decim M=2", "complex_float32", "COMPLEX", 63, M=2, plan="CF32_DECIM"),
    R("cf32 decim M=4", "complex_float32", "REAL", 100, M=4, plan="CF32_DECIM"),
    R("cf32 decim M=8", "complex_float32", "COMPLEX", 255, M=8, plan="CF32_DECIM"),
    R("cf32 decim M=8 K=2049", "complex_float32", "COMPLEX", 2049, M=8, plan="CF32_DECIM"),
    R("cf32 decim M=16", "complex_float32", "COMPLEX", 255, M=16, plan="CF32_DECIM"),
    R("cf32 decim M=160 (16-fold, one in 10 stored)", "complex_float32", "COMPLEX", 1000, M=160, plan="CF32_DECIM"),
    R("cf32 poly strided M=3", "complex_float32", "COMPLEX", 100, M=3, plan="CF32_POLY"),
    R("cf32 poly strided M=6 (2-fold: not folded)", "complex_float32", "REAL", 100, M=6, plan="CF32_POLY"),
    R("cf32 poly strided L=3 M=2", "complex_float32", "COMPLEX", 61, L=3, M=2, plan="CF32_POLY"),
    # -- complex_float32 interpolating: the replicated spectrum (CF32_INTERP, L in 2/4/8/16), polyphase rows otherwise --
    R("cf32 interp L=2", "complex_float32", "COMPLEX", 64, L=2, plan="CF32_INTERP"),
    R("cf32 interp L=4 K=513 (kov_in = 512, at its bound)", "complex_float32", "COMPLEX", 2049, L=4, plan="CF32_INTERP"),
    R("cf32 interp L=8", "complex_float32", "COMPLEX", 200, L=8, plan="CF32_INTERP"),
    R("cf32 interp L=16 K=129 (kov_in = 128 at its bound, 2049 taps)", "complex_float32", "REAL", 2049, L=16, plan="CF32_INTERP"),
    R("cf32 poly rows L=16 2050 taps (past the replicated plan)", "complex_float32", "REAL", 2050, L=16, plan="CF32_OLS4096_ROWS"),
    R("cf32 poly rows L=3 M=1", "complex_float32", "COMPLEX", 150, L=3, plan="CF32_OLS4096_ROWS"),
    # -- float32 (and complex_float32) long rows / long decimators: the partitioned kernel --
    R("cf32 upols rows L=2 K=2050", "complex_float32", "COMPLEX", 4100, L=2, bar=2 * TOL, plan="UPOLS_ROWS"),
    R("cf32 upols decim M=3 K=3000", "complex_float32", "COMPLEX", 3000, M=3, bar=2 * TOL, plan="UPOLS_DECIM"),
    R("f32 upols rows L=3 K=2050", "float32", "REAL", 6150, L=3, bar=2 * TOL, plan="UPOLS_ROWS"),
    R("f32 upols decim M=2 K=16", "float32", "REAL", 16, M=2, bar=2 * TOL, plan="UPOLS_DECIM"),
    R("f32 generic M=2 K=15 (below the decimating plan)", "float32", "REAL", 15, M=2, want="DIRECT", plan="GENERIC"),
    # -- float32, M = L = 1: two real blocks per transform, beyond 2049 taps the halves side by side --
    R("f32 sliding K=1", "float32", "REAL", 1, want="DIRECT", plan="SLIDE"),
    R("f32 real ols K=2049", "float32", "REAL", 2049, plan="F32_OLS4096"),
    R("f32 real ols partitioned K=2050", "float32", "REAL", 2050, bar=3 * TOL, plan="F32_UPOLS"),
    # -- float32 interpolating rows on the float kernel (F32_OLS4096_ROWS, 16 <= K <= 2049 under AUTO) --
    R("f32 generic L=3 K=15 (below the interpolating rows)", "float32", "REAL", 45, L=3, want="DIRECT", plan="GENERIC"),
    R("f32 interp rows L=3 K=16", "float32", "REAL", 46, L=3, plan="F32_OLS4096_ROWS"),
    R("f32 interp rows L=5 M=3 K=16", "float32", "REAL", 80, L=5, M=3, plan="F32_OLS4096_ROWS"),
    R("f32 interp rows L=5 M=3 K=2049", "float32", "REAL", 10245, L=5, M=3, plan="F32_OLS4096_ROWS"),
    # -- complex_float64 (CF64_OLS from K = 4, M > 1 from 16; CF64_OLS_ROWS to L = 64) --
    R("cf64 sliding K=3", "complex_float64", "COMPLEX", 3, want="DIRECT", plan="SLIDE"),
    R("cf64 ols K=4", "complex_float64", "COMPLEX", 4, plan="CF64_OLS"),
    R("cf64 ols K=2049 (4096 block)", "complex_float64", "REAL", 2049, plan="CF64_OLS"),
    R("cf64 ols K=2050 (8192 block)", "complex_float64", "COMPLEX", 2050, plan="CF64_OLS"),
    R("cf64 ols K=4097", "complex_float64", "COMPLEX", 4097, plan="CF64_OLS"),
    R("cf64 sliding K=4098", "complex_float64", "COMPLEX", 4098, want="DIRECT", plan="SLIDE"),
    R("cf64 generic M=2 K=15", "complex_float64", "COMPLEX", 15, M=2, want="DIRECT", plan="GENERIC"),
    R("cf64 ols decim M=2 K=16", "complex_float64", "COMPLEX", 16, M=2, plan="CF64_OLS"),
    R("cf64 ols decim M=65535", "complex_float64", "COMPLEX", 16, M=65535, plan="CF64_OLS"),
    R("cf64 generic M=65536 (past the decimating plans)", "complex_float64", "COMPLEX", 16, M=65536, want="DIRECT", plan="GENERIC"),
    R("cf64 interp64 L=64", "complex_float64", "COMPLEX", 1280, L=64, plan="CF64_OLS_ROWS"),
    R("cf64 generic L=65", "complex_float64", "COMPLEX", 1300, L=65, want="DIRECT", plan="GENERIC"),
    # -- complex_int16 (CF64_OLS from 64 taps while ||h_q||^2 < 2^44; the packed dot-product kernel below) --
    R("ci16 dot2 K=40", "complex_int16", "COMPLEX", 40, want="EXACT", tapgen="q16", plan="DOT2"),
    R("ci16 sliding K=63 real taps", "complex_int16", "REAL", 63, want="EXACT", plan="SLIDE"),
    R("ci16 ols K=64", "complex_int16", "COMPLEX", 64, plan="CF64_OLS"),
    R("ci16 ols K=2049", "complex_int16", "COMPLEX", 2049, plan="CF64_OLS"),
    R("ci16 ols K=2050", "complex_int16", "COMPLEX", 2050, plan="CF64_OLS"),
    R("ci16 ols K=4097", "complex_int16", "REAL", 4097, plan="CF64_OLS"),
    R("ci16 dot2 K=4098", "complex_int16", "COMPLEX", 4098, want="EXACT", plan="DOT2"),
    R("ci16 ols ||h_q||^2 below 2^44", "complex_int16", "COMPLEX", 64, tapgen=5.6 + 5.6j, plan="CF64_OLS"),
    R("ci16 sliding ||h_q||^2 above 2^44", "complex_int16", "COMPLEX", 64, want="EXACT", tapgen=5.7 + 5.7j, plan="SLIDE"),
    R("ci16 generic M=2 K=31", "complex_int16", "COMPLEX", 31, M=2, want="EXACT", plan="GENERIC"),
    R("ci16 ols decim M=2 K=32", "complex_int16", "COMPLEX", 32, M=2, plan="CF64_OLS"),
    R("ci16 interp64 L=64", "complex_int16", "COMPLEX", 1280, L=64, plan="CF64_OLS_ROWS"),
    R("ci16 interp64 L=3 M=2", "complex_int16", "COMPLEX", 60, L=3, M=2, plan="CF64_OLS_ROWS"),
    # -- complex_int8 (CF64_OLS from 96 taps) --
    R("ci8 dot2 K=40", "complex_int8", "COMPLEX", 40, want="EXACT", plan="DOT2"),
    R("ci8 dot2 K=95", "complex_int8", "COMPLEX", 95, want="EXACT", plan="DOT2"),
    R("ci8 ols K=96", "complex_int8", "COMPLEX", 96, plan="CF64_OLS"),
    R("ci8 interp64 L=64", "complex_int8", "COMPLEX", 1280, L=64, plan="CF64_OLS_ROWS"),
    R("ci8 generic L=65", "complex_int8", "COMPLEX", 1300, L=65, want="EXACT", plan="GENERIC"),
    # -- REAL float64 / int16 / int8 on the double pipeline (REAL64_OLS from 24 / 48 taps, M > 1 from 16; REAL64_OLS_ROWS) --
    R("f64 sliding K=23", "float64", "REAL", 23, want="DIRECT", plan="SLIDE"),
    R("f64 real ols K=24", "float64", "REAL", 24, plan="REAL64_OLS"),
    R("f64 real ols K=4097 (8192 block)", "float64", "REAL", 4097, plan="REAL64_OLS"),
    R("f64 sliding K=4098", "float64", "REAL", 4098, want="DIRECT", plan="SLIDE"),
    R("f64 real ols decim M=3 K=16", "float64", "REAL", 16, M=3, plan="REAL64_OLS"),
    R("f64 interp real L=3", "float64", "REAL", 120, L=3, plan="REAL64_OLS_ROWS"),
    R("i16 sliding K=47", "int16", "REAL", 47, want="EXACT", plan="SLIDE"),
    R("i16 real ols K=48", "int16", "REAL", 48, plan="REAL64_OLS"),
    R("i16 real ols K=2049", "int16", "REAL", 2049, plan="REAL64_OLS"),
    R("i16 real ols K=2050", "int16", "REAL", 2050, plan="REAL64_OLS"),
    R("i16 real ols K=4097", "int16", "REAL", 4097, plan="REAL64_OLS"),
    R("i16 sliding K=4098", "int16", "REAL", 4098, want="EXACT", plan="SLIDE"),
    R("i16 interp real L=4 M=3", "int16", "REAL", 80, L=4, M=3, plan="REAL64_OLS_ROWS"),
    R("i8 sliding K=47", "int8", "REAL", 47, want="EXACT", plan="SLIDE"),
    R("i8 real ols K=48", "int8", "REAL", 48, plan="REAL64_OLS"),
    R("i8 interp real L=2", "int8", "REAL", 32, L=2, plan="REAL64_OLS_ROWS"),
    R("i8 generic L=2 K=15", "int8", "REAL", 30, L=2, want="EXACT", plan="GENERIC"),
    # -- the wide integer types: the time-domain kernels only --
    R("ci32 sliding K=3", "complex_int32", "COMPLEX", 3, want="EXACT", plan="SLIDE"),
    R("ci32 generic L=3 M=2", "complex_int32", "COMPLEX", 13, L=3, M=2, want="EXACT", plan="GENERIC"),
    R("i64 sliding K=3", "int64", "REAL", 3, want="EXACT", plan="SLIDE"),
    R("ci64 generic L=2 M=3", "complex_int64", "REAL", 9, L=2, M=3, want="EXACT", plan="GENERIC"),
]
IDS = [r.name for r in PLANS]


def _K(row):
    return -(-row.ntaps // row.L)


def _taps(row):
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    n, cplx = row.ntaps, row.taps == "COMPLEX"
    if isinstance(row.tapgen, complex):                            # every tap the same: a chosen ||h_q||
        return np.full(n, row.tapgen) if cplx else np.full(n, row.tapgen.real)
    if row.tapgen == "q16":                                        # Q16.16 images inside +-32767 (the packed kernel's range)
        return rng.uniform(-0.49, 0.49, n) + (1j * rng.uniform(-0.49, 0.49, n) if cplx else 0)
    t = rng.normal(size=n) / np.sqrt(max(1, _K(row)))
    if cplx:
        t = t + 1j * rng.normal(size=n) / np.sqrt(max(1, _K(row)))
    return t * 0.9


def _stream(row, o, scalar, cplx):
    """(input, n_in, n_out): a few 4096-sample blocks of input with ragged ends (a few hundred iterations for 64-fold
    interpolation, three outputs for the largest decimations)"""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()) + 1)
    K = _K(row)
    it = 3 * row.M + 1234 if row.M >= 1000 else 777 + row.M // 2 if row.L >= 32 else 2 * 4096 + 777 + row.M // 2
    n_in = K - 1 + it
    n_out = (it // row.M) * row.L
    dt = o.NP_SCALAR[scalar]
    shape = (n_in, 2) if cplx else (n_in,)
    if np.issubdtype(dt, np.floating):
        x = rng.uniform(-1, 1, shape).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    return x, n_in, n_out


def _configure(f, row, q=None):
    """the handle's settings through the setters alone"""
    from oracle import oracle as o
    from pothoscomms_amd import _lib
    f.set_taps(_taps(row))
    f.set_decimation(row.M)
    f.set_interpolation(row.L)
    f.set_algo(getattr(_lib, "FIR_" + row.algo))
    if f.scalar not in (o.F32, o.F64):          # integer element types: the Q-format reading is one more input of the tables
        f.set_qformat(q)


def _make(dev, row, q=None):
    f = dev.FirFilter(row.dtype, row.taps)
    _configure(f, row, q)
    return f
