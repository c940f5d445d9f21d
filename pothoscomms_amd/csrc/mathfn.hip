// mathfn.hip -- the real-valued function blocks of the reference's math/ (DESIGN.md 20):
//   /comms/exp exp2 exp10 expm1 expN            math/Exp.cpp (Exp10.hpp.in)
//   /comms/log log2 log10 log1p logN            math/Log.cpp
//   /comms/pow                                  math/Pow.cpp
//   /comms/sqrt cbrt nth_root                   math/Root.cpp
//   /comms/rsqrt sinc sigmoid                   math/RSqrt.cpp (RSqrt.hpp), math/Sinc.cpp, math/Sigmoid.cpp
//   /comms/trigonometric, 24 operations         math/Trigonometric.cpp
// float32 and float64, the reference's scalar loops (its branches without POTHOS_XSIMD).
//
// THE ARITHMETIC.  The reference's results are glibc's, these are the ROCm device library's: there is no bit parity to be had, and the
// bar is a truth both approximate.  A float64 element is the device library's double function of it.  A float32
// element is widened, goes through THE SAME double expression and is rounded once: the result is then the correctly rounded value of the
// exact expression unless the double result lies within its own error of a float32 rounding boundary, whatever that error is.  Three
// results have one right answer and are held to equality: sqrt in both types (a correctly rounded double root rounded to float32 IS the
// correctly rounded float32 root, 53 >= 2 * 24 + 2), rsqrt on float64 (a correctly rounded root and a correctly rounded division) and
// rsqrt on float32, which in the reference is not 1 / sqrt but the bit trick of RSqrt.hpp:13-25 -- integer and float32 arithmetic,
// unfused here as on x86-64 (-ffp-contract=off).
//
// ONE SHAPE, as logic.hip's: a buffer is a run of 16-byte units counted from its first byte, at any byte address (unit_io.hpp); a lane
// owns output unit u, four float32 or two float64.  A chunk of kBlock units that lies whole inside the buffer takes the unguarded
// 16-byte load and store, the chunk a buffer ends in goes through load_unit / store_unit, which touch single bytes in the last unit
// only.  Unlike logic.hip's kernel this one has ONE call site of the functor between the two kinds of load and store: pow or tan is
// several hundred instructions an element, and a second inlined copy for the tail would double the kernel for nothing (a lane past the
// end evaluates zeros and stores nothing).  One instantiation per function and type: no switch in a kernel, so sqrt does not carry the
// registers of pow.  `out` may be exactly `in`: a lane reads its own unit before it writes it and touches no other.  Every index 64-bit.
#include "fn_kernel.hpp"       // mathfn_kernel, apply1 and launch_fn: shared with specfn.hip

namespace pcx {
namespace {

// ---- the expressions, each as the reference writes it (file:line of its scalar loop) ----
#define PCX_FN1(NAME, EXPR)                                              \
    struct NAME {                                                        \
        __device__ __forceinline__ double operator()(double x) const { return EXPR; } \
    }
PCX_FN1(FExp, ::exp(x));                    // Exp.cpp:68
PCX_FN1(FExp2, ::exp2(x));                  // Exp.cpp:77
PCX_FN1(FExp10, ::exp10(x));                // Exp10.hpp.in:21-32: exp10f / exp10 where the C library has them, as glibc does
// (C's expm1 and log1p return a zero with its sign; the device library's return +0 for -0: MEASURED)
PCX_FN1(FExpm1, x == 0.0 ? x : ::expm1(x));  // Exp.cpp:92
PCX_FN1(FLog, ::log(x));                    // Log.cpp:82
PCX_FN1(FLog2, ::log2(x));                  // Log.cpp:91
PCX_FN1(FLog10, ::log10(x));                // Log.cpp:100
PCX_FN1(FLog1p, x == 0.0 ? x : ::log1p(x));  // Log.cpp:109
PCX_FN1(FSqrt, ::sqrt(x));                  // Root.cpp:94
PCX_FN1(FCbrt, ::cbrt(x));                  // Root.cpp:103
PCX_FN1(FSinc, ::fabs(x) < 1e-6 ? 1.0 : ::sin(x) / x);   // Sinc.cpp:36-37: the comparison in double, a NaN goes the second way
PCX_FN1(FSigmoid, 1.0 / (1.0 + ::exp(-x)));               // Sigmoid.cpp:36
// Trigonometric.cpp:178-385: the reciprocal functions are 1 / f(x), the inverse reciprocal ones f(1 / x)
PCX_FN1(FCos, ::cos(x));
PCX_FN1(FSin, ::sin(x));
PCX_FN1(FTan, ::tan(x));
PCX_FN1(FSec, 1.0 / ::cos(x));
PCX_FN1(FCsc, 1.0 / ::sin(x));
PCX_FN1(FCot, 1.0 / ::tan(x));
PCX_FN1(FAcos, ::acos(x));
PCX_FN1(FAsin, ::asin(x));
PCX_FN1(FAtan, ::atan(x));
PCX_FN1(FAsec, ::acos(1.0 / x));
PCX_FN1(FAcsc, ::asin(1.0 / x));
PCX_FN1(FAcot, ::atan(1.0 / x));
PCX_FN1(FCosh, ::cosh(x));
PCX_FN1(FSinh, ::sinh(x));
PCX_FN1(FTanh, ::tanh(x));
PCX_FN1(FSech, 1.0 / ::cosh(x));
PCX_FN1(FCsch, 1.0 / ::sinh(x));
PCX_FN1(FCoth, 1.0 / ::tanh(x));
PCX_FN1(FAcosh, ::acosh(x));
PCX_FN1(FAsinh, ::asinh(x));
PCX_FN1(FAtanh, ::atanh(x));
PCX_FN1(FAsech, ::acosh(1.0 / x));
PCX_FN1(FAcsch, ::asinh(1.0 / x));
PCX_FN1(FAcoth, ::atanh(1.0 / x));
#undef PCX_FN1

// RSqrt.hpp:13-25 resp. :39
struct FRsqrt {
    __device__ __forceinline__ double operator()(double x) const { return 1.0 / ::sqrt(x); }
    __device__ __forceinline__ float f32(float f) const
    {
        const uint32_t u = 0x5F1FFFF9u - (__float_as_uint(f) >> 1);
        const float f2 = __uint_as_float(u);
        return 0.703952253f * f2 * (2.38924456f - f * f2 * f2);
    }
};

// the parameterised ones; the parameter is a value of the element type, carried as the double it widens to
struct FExpN {          // Exp.cpp:101  pow(base, x)
    double base;
    __device__ __forceinline__ double operator()(double x) const { return ::pow(base, x); }
};
struct FLogN {          // Log.cpp:118  log(x) / log(base)
    double base;
    __device__ __forceinline__ double operator()(double x) const { return ::log(x) / ::log(base); }
};
struct FPow {           // Pow.cpp:40  pow(x, exponent)
    double e;
    __device__ __forceinline__ double operator()(double x) const { return ::pow(x, e); }
};
// Root.cpp:119 and :131: the exponent is the DOUBLE 1.0 / root and the pow the double one, for float32 too; ODD (:164, exactly when
// fmod(root, 2) == 1) mirrors a negative input, f = (x < 0) ? -1 : 1 (:44), so -0.0 and a NaN keep f = 1
template <bool ODD>
struct FNthRoot {
    double inv;
    __device__ __forceinline__ double operator()(double x) const
    {
        if (!ODD) return ::pow(x, inv);
        const double f = x < 0 ? -1.0 : 1.0;
        return ::pow(x * f, inv) * f;
    }
};

template <typename T>
int launch_mathfn_t(int fn, double p, const void *in, void *out, size_t n, hipStream_t st)
{
    switch (fn) {
#define PCX_CASE(CODE, F) case CODE: return launch_fn<T>(in, out, n, F{}, st)
    PCX_CASE(PCX_MATH_EXP, FExp);
    PCX_CASE(PCX_MATH_EXP2, FExp2);
    PCX_CASE(PCX_MATH_EXP10, FExp10);
    PCX_CASE(PCX_MATH_EXPM1, FExpm1);
    PCX_CASE(PCX_MATH_LOG, FLog);
    PCX_CASE(PCX_MATH_LOG2, FLog2);
    PCX_CASE(PCX_MATH_LOG10, FLog10);
    PCX_CASE(PCX_MATH_LOG1P, FLog1p);
    PCX_CASE(PCX_MATH_SQRT, FSqrt);
    PCX_CASE(PCX_MATH_CBRT, FCbrt);
    PCX_CASE(PCX_MATH_RSQRT, FRsqrt);
    PCX_CASE(PCX_MATH_SINC, FSinc);
    PCX_CASE(PCX_MATH_SIGMOID, FSigmoid);
    PCX_CASE(PCX_MATH_COS, FCos);
    PCX_CASE(PCX_MATH_SIN, FSin);
    PCX_CASE(PCX_MATH_TAN, FTan);
    PCX_CASE(PCX_MATH_SEC, FSec);
    PCX_CASE(PCX_MATH_CSC, FCsc);
    PCX_CASE(PCX_MATH_COT, FCot);
    PCX_CASE(PCX_MATH_ACOS, FAcos);
    PCX_CASE(PCX_MATH_ASIN, FAsin);
    PCX_CASE(PCX_MATH_ATAN, FAtan);
    PCX_CASE(PCX_MATH_ASEC, FAsec);
    PCX_CASE(PCX_MATH_ACSC, FAcsc);
    PCX_CASE(PCX_MATH_ACOT, FAcot);
    PCX_CASE(PCX_MATH_COSH, FCosh);
    PCX_CASE(PCX_MATH_SINH, FSinh);
    PCX_CASE(PCX_MATH_TANH, FTanh);
    PCX_CASE(PCX_MATH_SECH, FSech);
    PCX_CASE(PCX_MATH_CSCH, FCsch);
    PCX_CASE(PCX_MATH_COTH, FCoth);
    PCX_CASE(PCX_MATH_ACOSH, FAcosh);
    PCX_CASE(PCX_MATH_ASINH, FAsinh);
    PCX_CASE(PCX_MATH_ATANH, FAtanh);
    PCX_CASE(PCX_MATH_ASECH, FAsech);
    PCX_CASE(PCX_MATH_ACSCH, FAcsch);
    PCX_CASE(PCX_MATH_ACOTH, FAcoth);
#undef PCX_CASE
    case PCX_MATH_EXPN: return launch_fn<T>(in, out, n, FExpN{p}, st);
    case PCX_MATH_LOGN: return launch_fn<T>(in, out, n, FLogN{p}, st);
    case PCX_MATH_POW: return launch_fn<T>(in, out, n, FPow{p}, st);
    case PCX_MATH_NTH_ROOT:
        if (std::fmod((T)p, T(2)) == 1) return launch_fn<T>(in, out, n, FNthRoot<true>{1.0 / p}, st);
        return launch_fn<T>(in, out, n, FNthRoot<false>{1.0 / p}, st);
    }
    set_error("math function: unknown function %d", fn);
    return PCX_ERR_ARG;
}

}  // namespace

int launch_mathfn(int scalar, int fn, double param, const void *in, void *out, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    switch (scalar) {
    case PCX_F64: return launch_mathfn_t<double>(fn, param, in, out, n, st);
    case PCX_F32: return launch_mathfn_t<float>(fn, param, in, out, n, st);
    }
    set_error("math function: unsupported type (scalar %d)", scalar);
    return PCX_ERR_ARG;
}

}  // namespace pcx
