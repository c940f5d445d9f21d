// fn_kernel.hpp -- the one-input map of the function blocks, shared by mathfn.hip and specfn.hip: a lane
// owns a 16-byte unit at any byte address, one call site of the functor, one instantiation per functor and type (mathfn.hip's header
// comment has the reasons).  The names stay internal to the translation unit that includes it.
#pragma once
#include "pcx_internal.hpp"
#include "unit_io.hpp"

#include <type_traits>

namespace pcx {
namespace {

constexpr int kBlock = 256;

// a functor is a double expression; one that is NOT that for float32 says so and brings its own float32 form
template <typename F, typename = void>
struct HasF32 : std::false_type {};
template <typename F>
struct HasF32<F, decltype((void)&F::f32)> : std::true_type {};

template <typename T, typename F>
__device__ __forceinline__ T apply1(const F &f, T x)
{
    if constexpr (std::is_same<T, float>::value && HasF32<F>::value) return f.f32(x);
    else return (T)f((double)x);
}

template <typename T, typename F>
__global__ __launch_bounds__(kBlock) void mathfn_kernel(const unsigned char *in, unsigned char *out, int64_t n, F f)
{
    constexpr int N = 16 / (int)sizeof(T);
    const int64_t nunits = (n + 15) / 16;
    const int64_t nchunks = (nunits + kBlock - 1) / kBlock;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t unit = c * kBlock + threadIdx.x;
        const bool whole = (c + 1) * kBlock * 16 <= n;          // (the same for every lane of the workgroup)
        uint4 v = make_uint4(0, 0, 0, 0);
        if (whole) v = nt_load16_any(in + 16 * unit);
        else if (unit < nunits) v = load_unit(in, 16 * unit, n);
        T x[N], y[N];
        __builtin_memcpy(x, &v, 16);
#pragma unroll
        for (int k = 0; k < N; k++) y[k] = apply1<T, F>(f, x[k]);
        __builtin_memcpy(&v, y, 16);
        if (whole) nt_store16_any(out + 16 * unit, v);
        else if (unit < nunits) store_unit(out, 16 * unit, n, v);
    }
}

template <typename T, typename F>
int launch_fn(const void *in, void *out, size_t n, F f, hipStream_t st)
{
    const size_t bytes = n * sizeof(T), nunits = (bytes + 15) / 16;
    const unsigned grid = stream_grid(nunits, kBlock);
    hipLaunchKernelGGL((mathfn_kernel<T, F>), dim3(grid), dim3(kBlock), 0, st, static_cast<const unsigned char *>(in),
                       static_cast<unsigned char *>(out), (int64_t)bytes, f);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace
}  // namespace pcx
