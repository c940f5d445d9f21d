// specfn.hip -- the special-function blocks of the reference's math/ (DESIGN.md 21), which complete that directory:
//   /comms/gamma lngamma                        math/Gamma.cpp:27-53       std::tgamma, std::lgamma
//   /comms/erf erfc                             math/ErrorFunction.cpp:27-53   std::erf, std::erfc
//   /comms/beta                                 math/Beta.cpp:31-43        std::beta == exp(lgamma(a) + lgamma(b) - lgamma(a + b))
//   /comms/modf                                 math/ModF.cpp:31-38        frac = std::modf(x, &int)
// float32 and float64, the reference's scalar loops (its branches without POTHOS_XSIMD).
//
// THE ARITHMETIC is mathfn.hip's: a float64 element is the device library's double function of it, a float32 element is widened, goes
// through THE SAME double expression and is rounded once.  The bar is the correctly rounded value of the exact expression (DESIGN.md
// 21), not glibc's bits.  modf has one right answer and is evaluated in the element type: a truncation and an exact difference.
//
// THREE SHAPES, all of fn_kernel.hpp's discipline: a buffer is a run of 16-byte units counted from its first byte, at any byte address;
// a lane owns unit u of every buffer of the call; a chunk that lies whole inside the buffers takes the unguarded 16-byte accesses, the
// chunk they end in goes through load_unit / store_unit; one call site of the functor; a lane past the end evaluates zeros and stores
// nothing; every index 64-bit.
//   mathfn_kernel<T, F>   one input, one output (fn_kernel.hpp): gamma, lngamma, erf, erfc
//   map2_kernel<T, F>     two inputs, one output: beta.  `out` may be exactly in0 or exactly in1 (a lane reads its own unit of both before
//                         it writes it); the inputs may overlap each other in any way, they are only read
//   split_kernel<T>       one input, two outputs: modf.  Either output may be exactly `in`; the outputs share no byte
#include "fn_kernel.hpp"

namespace pcx {
namespace {

// ---- the expressions ----
// The device library's tgamma, lgamma, erf and erfc were MEASURED on the special inputs of the fixture (zeros of both signs,
// poles, infinities, the overflow and underflow thresholds) and return what C prescribes at every one of them -- unlike its expm1 and
// log1p -- so the functors are the bare calls.
struct FGamma {         // Gamma.cpp:34  std::tgamma
    __device__ __forceinline__ double operator()(double x) const { return ::tgamma(x); }
};
struct FLnGamma {       // Gamma.cpp:48  std::lgamma
    __device__ __forceinline__ double operator()(double x) const { return ::lgamma(x); }
};
struct FErf {           // ErrorFunction.cpp:34  std::erf
    __device__ __forceinline__ double operator()(double x) const { return ::erf(x); }
};
struct FErfc {          // ErrorFunction.cpp:48  std::erfc
    __device__ __forceinline__ double operator()(double x) const { return ::erfc(x); }
};
// Beta.cpp:37 std::beta, which in libstdc++ is the expression of :39 in the element type (and a NaN for a NaN): the sign of a negative
// argument's gamma is lost, as there.  Here the expression is the double one for both types; a + b of two float32 values is exact in
// double wherever their exponents lie within 29 of each other.  A log-gamma term beyond the range of float32 (an argument above 4e36)
// is the infinity it is in the reference's float32 expression, so beta(FLT_MAX, 1) is inf - inf there and here.
template <typename T>
struct FBeta {
    static __device__ __forceinline__ double term(double x)
    {
        const double l = ::lgamma(x);
        if (std::is_same<T, float>::value && __builtin_fabs(l) > 3.4028234663852886e38) return __builtin_copysign(__builtin_inf(), l);
        return l;
    }
    // THE LARGE ARGUMENT.  The value is the exact expression's; evaluated term by term it is lost once the larger argument x is large:
    // lgamma(x) and lgamma(x + y) are then huge and nearly equal, and their difference keeps only the absolute error of their last
    // place (3e-5 at x = 1e10, where the float32 result would be tens of units off).  From x = 1024 on the difference is taken from
    // Stirling's series instead, whose leading terms cancel in closed form:
    //     lgamma(x) - lgamma(x + y) = y - y ln x - (x + y - 1/2) log1p(y / x) + S(x) - S(x + y),  S(z) = 1/(12 z) - 1/(360 z^3) + 1/(1260 z^5)
    // (the next term of S is below 1/(1680 z^7) < 1e-24 there).  Every term is of the size of y ln x, not of x ln x.  Where a
    // log-gamma term of the expression is not finite in the element type the expression's own result stands, as in the reference.
    static __device__ __forceinline__ double stirling_tail(double z)
    {
        const double r = 1.0 / z, r2 = r * r;
        return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0)));
    }
    __device__ __forceinline__ double operator()(double a, double b) const
    {
        const double la = term(a), lb = term(b);
        const bool a_larger = a > b;
        const double x = a_larger ? a : b, y = a_larger ? b : a, lx = a_larger ? la : lb, ly = a_larger ? lb : la;
        if (x >= 1024.0 && y > 0.0 && __builtin_isfinite(lx)) {          // (a NaN fails one of the comparisons)
            const double d = (y - y * ::log(x)) - (x + y - 0.5) * ::log1p(y / x) + (stirling_tail(x) - stirling_tail(x + y));
            return ::exp(ly + d);
        }
        return ::exp(la + lb - term(a + b));
    }
};
// ModF.cpp:36: the integral part is x truncated (an infinity stays one), the fraction x less that, exactly, with the sign of x -- so
// -0.0 for a negative integer and for -inf, where the difference would be a NaN
template <typename T>
__device__ __forceinline__ void modf1(T x, T &ip, T &fp)
{
    if constexpr (std::is_same<T, float>::value) {
        ip = __builtin_truncf(x);
        fp = __builtin_isinf(x) ? __builtin_copysignf(0.0f, x) : __builtin_copysignf(x - ip, x);
    } else {
        ip = __builtin_trunc(x);
        fp = __builtin_isinf(x) ? __builtin_copysign(0.0, x) : __builtin_copysign(x - ip, x);
    }
}

// ---- two inputs, one output ----
template <typename T, typename F>
__global__ __launch_bounds__(kBlock) void map2_kernel(const unsigned char *in0, const unsigned char *in1, unsigned char *out, int64_t n, F f)
{
    constexpr int N = 16 / (int)sizeof(T);
    const int64_t nunits = (n + 15) / 16;
    const int64_t nchunks = (nunits + kBlock - 1) / kBlock;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t unit = c * kBlock + threadIdx.x;
        const bool whole = (c + 1) * kBlock * 16 <= n;          // (the same for every lane of the workgroup)
        uint4 v0 = make_uint4(0, 0, 0, 0), v1 = make_uint4(0, 0, 0, 0);
        if (whole) {
            v0 = nt_load16_any(in0 + 16 * unit);
            v1 = nt_load16_any(in1 + 16 * unit);
        } else if (unit < nunits) {
            v0 = load_unit(in0, 16 * unit, n);
            v1 = load_unit(in1, 16 * unit, n);
        }
        T a[N], b[N], y[N];
        __builtin_memcpy(a, &v0, 16);
        __builtin_memcpy(b, &v1, 16);
#pragma unroll
        for (int k = 0; k < N; k++) y[k] = (T)f((double)a[k], (double)b[k]);
        __builtin_memcpy(&v0, y, 16);
        if (whole) nt_store16_any(out + 16 * unit, v0);
        else if (unit < nunits) store_unit(out, 16 * unit, n, v0);
    }
}

// ---- one input, two outputs ----
template <typename T>
__global__ __launch_bounds__(kBlock) void split_kernel(const unsigned char *in, unsigned char *out0, unsigned char *out1, int64_t n)
{
    constexpr int N = 16 / (int)sizeof(T);
    const int64_t nunits = (n + 15) / 16;
    const int64_t nchunks = (nunits + kBlock - 1) / kBlock;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t unit = c * kBlock + threadIdx.x;
        const bool whole = (c + 1) * kBlock * 16 <= n;          // (the same for every lane of the workgroup)
        uint4 v = make_uint4(0, 0, 0, 0), w;
        if (whole) v = nt_load16_any(in + 16 * unit);
        else if (unit < nunits) v = load_unit(in, 16 * unit, n);
        T x[N], y0[N], y1[N];
        __builtin_memcpy(x, &v, 16);
#pragma unroll
        for (int k = 0; k < N; k++) modf1<T>(x[k], y0[k], y1[k]);
        __builtin_memcpy(&v, y0, 16);
        __builtin_memcpy(&w, y1, 16);
        if (whole) {
            nt_store16_any(out0 + 16 * unit, v);
            nt_store16_any(out1 + 16 * unit, w);
        } else if (unit < nunits) {
            store_unit(out0, 16 * unit, n, v);
            store_unit(out1, 16 * unit, n, w);
        }
    }
}

template <typename T>
int launch_specfn_t(int fn, const void *in, void *out, size_t n, hipStream_t st)
{
    switch (fn) {
    case PCX_SPEC_GAMMA: return launch_fn<T>(in, out, n, FGamma{}, st);
    case PCX_SPEC_LNGAMMA: return launch_fn<T>(in, out, n, FLnGamma{}, st);
    case PCX_SPEC_ERF: return launch_fn<T>(in, out, n, FErf{}, st);
    case PCX_SPEC_ERFC: return launch_fn<T>(in, out, n, FErfc{}, st);
    }
    set_error("special function: unknown function %d", fn);
    return PCX_ERR_ARG;
}

template <typename T>
int launch_beta_t(const void *in0, const void *in1, void *out, size_t n, hipStream_t st)
{
    const size_t bytes = n * sizeof(T), nunits = (bytes + 15) / 16;
    hipLaunchKernelGGL((map2_kernel<T, FBeta<T>>), dim3(stream_grid(nunits, kBlock)), dim3(kBlock), 0, st, static_cast<const unsigned char *>(in0),
                       static_cast<const unsigned char *>(in1), static_cast<unsigned char *>(out), (int64_t)bytes, FBeta<T>{});
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

template <typename T>
int launch_modf_t(const void *in, void *out_int, void *out_frac, size_t n, hipStream_t st)
{
    const size_t bytes = n * sizeof(T), nunits = (bytes + 15) / 16;
    hipLaunchKernelGGL((split_kernel<T>), dim3(stream_grid(nunits, kBlock)), dim3(kBlock), 0, st, static_cast<const unsigned char *>(in),
                       static_cast<unsigned char *>(out_int), static_cast<unsigned char *>(out_frac), (int64_t)bytes);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace

int launch_specfn(int scalar, int fn, const void *in, void *out, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    switch (scalar) {
    case PCX_F64: return launch_specfn_t<double>(fn, in, out, n, st);
    case PCX_F32: return launch_specfn_t<float>(fn, in, out, n, st);
    }
    set_error("special function: unsupported type (scalar %d)", scalar);
    return PCX_ERR_ARG;
}

int launch_beta(int scalar, const void *in0, const void *in1, void *out, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    switch (scalar) {
    case PCX_F64: return launch_beta_t<double>(in0, in1, out, n, st);
    case PCX_F32: return launch_beta_t<float>(in0, in1, out, n, st);
    }
    set_error("beta: unsupported type (scalar %d)", scalar);
    return PCX_ERR_ARG;
}

int launch_modf(int scalar, const void *in, void *out_int, void *out_frac, size_t n, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    switch (scalar) {
    case PCX_F64: return launch_modf_t<double>(in, out_int, out_frac, n, st);
    case PCX_F32: return launch_modf_t<float>(in, out_int, out_frac, n, st);
    }
    set_error("modf: unsupported type (scalar %d)", scalar);
    return PCX_ERR_ARG;
}

}  // namespace pcx
