// arith_ops.hpp -- the element operators of /comms/arithmetic (arith.hip) and /comms/const_arithmetic (logic.hip): the C++ operators
// math/Arithmetic.cpp:70-110 applies, restated for the device type by type.  The derivation stands in arith.hip's header comment and in
// oracle/pcx_oracle.c (orc_arith).  Include from a translation unit built with -ffp-contract=off.
#pragma once
#include <type_traits>

#include "pcx.h"
#include "pcx_cplx.hpp"

namespace pcx {

// ---- promoted / division types per element type (see the header comment) ----
template <typename T> struct Prom {
    typedef typename std::conditional<(sizeof(T) < 4), int, typename std::make_unsigned<T>::type>::type P;   // + - *
    typedef typename std::conditional<(sizeof(T) < 4), int, T>::type D;                                      // /
};
template <typename D>
__device__ __forceinline__ D int_div(D a, D b)
{
    if (b == 0) return 0;
    if (std::is_signed<D>::value && sizeof(D) >= 4 && b == (D)-1) return (D)(0 - (typename std::make_unsigned<D>::type)a);   // wraps at MIN
    return (D)(a / b);
}

template <typename T, int OP, bool FLT = std::is_floating_point<T>::value>
struct RealOp;
template <typename T, int OP>
struct RealOp<T, OP, true> {
    __device__ void operator()(const T *a, const T *b, T *o) const
    {
        o[0] = OP == PCX_ARITH_ADD ? a[0] + b[0] : OP == PCX_ARITH_SUB ? a[0] - b[0] : OP == PCX_ARITH_MUL ? a[0] * b[0] : a[0] / b[0];
    }
};
template <typename T, int OP>
struct RealOp<T, OP, false> {
    __device__ void operator()(const T *a, const T *b, T *o) const
    {
        typedef typename Prom<T>::P P;
        typedef typename Prom<T>::D D;
        const P x = (P)a[0], y = (P)b[0];
        if (OP == PCX_ARITH_ADD) o[0] = (T)(P)(x + y);
        else if (OP == PCX_ARITH_SUB) o[0] = (T)(P)(x - y);
        else if (OP == PCX_ARITH_MUL) o[0] = (T)(P)(x * y);
        else o[0] = (T)int_div<D>((D)a[0], (D)b[0]);
    }
};

template <typename T, int OP, bool FLT = std::is_floating_point<T>::value>
struct CplxOp;
// complex<integer>: libstdc++ generic members
template <typename T, int OP>
struct CplxOp<T, OP, false> {
    __device__ void operator()(const T *a, const T *b, T *o) const
    {
        typedef typename Prom<T>::P P;
        typedef typename Prom<T>::D D;
        const P ar = (P)a[0], ai = (P)a[1], br = (P)b[0], bi = (P)b[1];
        if (OP == PCX_ARITH_ADD) { o[0] = (T)(P)(ar + br); o[1] = (T)(P)(ai + bi); }
        else if (OP == PCX_ARITH_SUB) { o[0] = (T)(P)(ar - br); o[1] = (T)(P)(ai - bi); }
        else if (OP == PCX_ARITH_MUL) { o[0] = (T)(P)(ar * br - ai * bi); o[1] = (T)(P)(ar * bi + ai * br); }
        else {
            const T r = (T)(P)(ar * br + ai * bi);
            const T nn = (T)(P)(br * br + bi * bi);
            const P num = (P)(ai * br - ar * bi);     // stays in the promoted type
            o[1] = (T)int_div<D>((D)num, (D)nn);
            o[0] = (T)int_div<D>((D)r, (D)nn);
        }
    }
};
template <int OP>
struct CplxOp<float, OP, true> {
    __device__ void operator()(const float *a, const float *b, float *o) const
    {
        if (OP == PCX_ARITH_ADD) { o[0] = a[0] + b[0]; o[1] = a[1] + b[1]; }
        else if (OP == PCX_ARITH_SUB) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; }
        else if (OP == PCX_ARITH_MUL) {
            const float ac = a[0] * b[0], bd = a[1] * b[1], ad = a[0] * b[1], bc = a[1] * b[0];
            float x = ac - bd, y = ad + bc;
            if (both_nan(x, y)) cmul_annex_g(a[0], a[1], b[0], b[1], x, y);   // __mulsc3's slow path
            o[0] = x; o[1] = y;
        } else {
            const double aa = a[0], bb = a[1], cc = b[0], dd = b[1];
            const double den = (cc * cc) + (dd * dd);
            float x = (float)(((aa * cc) + (bb * dd)) / den);
            float y = (float)(((bb * cc) - (aa * dd)) / den);
            if (both_nan(x, y)) cdiv_annex_g(a[0], a[1], b[0], b[1], x, y);   // __divsc3's
            o[0] = x; o[1] = y;
        }
    }
};
template <int OP>
struct CplxOp<double, OP, true> {
    __device__ void operator()(const double *x, const double *y, double *o) const
    {
        double a = x[0], b = x[1], c = y[0], d = y[1];
        if (OP == PCX_ARITH_ADD) { o[0] = a + c; o[1] = b + d; }
        else if (OP == PCX_ARITH_SUB) { o[0] = a - c; o[1] = b - d; }
        else if (OP == PCX_ARITH_MUL) {
            const double ac = a * c, bd = b * d, ad = a * d, bc = b * c;
            double x = ac - bd, y = ad + bc;
            if (both_nan(x, y)) cmul_annex_g(a, b, c, d, x, y);   // __muldc3's slow path
            o[0] = x; o[1] = y;
        } else {
            // libgcc's __divdc3 as shipped since GCC 12 (what the reference's operator/ calls; restated here and checked
            // bit for bit against this box's libgcc on 4 M wide-range and special operands): Smith's division with the
            // operands rescaled when the denominator is huge or tiny or a numerator part would underflow, and the other
            // order of operations when the ratio itself is subnormal
            constexpr double kBig = 1.7976931348623157e308 / 2, kMin = 2.2250738585072014e-308, kMin2 = 2.220446049250313e-16,
                             kScale = 1.0 / 2.220446049250313e-16, kMax2 = kBig * kMin2;
            double aa = a, bb = b, cc = c, dd = d;
            const bool first = fabs(cc) < fabs(dd);
            const double m = first ? fabs(dd) : fabs(cc);
            double f = 1.0;
            if (m >= kBig) f = 0.5;
            else if (m < kMin2) f = kScale;
            else if ((fabs(aa) < kMin && fabs(bb) < kMax2 && m < kMax2) || (fabs(bb) < kMin && fabs(aa) < kMax2 && m < kMax2)) f = kScale;
            aa *= f; bb *= f; cc *= f; dd *= f;
            double x, y;
            if (first) {
                const double ratio = cc / dd, den = (cc * ratio) + dd;
                if (fabs(ratio) > kMin) { x = ((aa * ratio) + bb) / den; y = ((bb * ratio) - aa) / den; }
                else { x = ((cc * (aa / dd)) + bb) / den; y = ((cc * (bb / dd)) - aa) / den; }
            } else {
                const double ratio = dd / cc, den = (dd * ratio) + cc;
                if (fabs(ratio) > kMin) { x = ((bb * ratio) + aa) / den; y = (bb - (aa * ratio)) / den; }
                else { x = ((dd * (bb / cc)) + aa) / den; y = (bb - (dd * (aa / cc))) / den; }
            }
            a = aa; b = bb; c = cc; d = dd;     // the slow path below sees the rescaled operands, as libgcc's does
            if (both_nan(x, y)) cdiv_annex_g(a, b, c, d, x, y);   // __divdc3's
            o[0] = x; o[1] = y;
        }
    }
};

}  // namespace pcx
