// probe.hip -- /comms/signal_probe (utility/SignalProbe.cpp:123-163): a stream cut into windows of W elements, each reduced to one
// pair of doubles: the last element (VALUE), sqrt(sum |x|^2 / N) (RMS) or sum x / N (MEAN).  The reference sums in stream order; here
// the sum runs over ONE FIXED TREE that depends on nothing but the element type and the number N of elements:
//   a window is read in 16-byte units from its own first byte, whatever that address is; unit u = 256 c + l lies in CHUNK c (256
//   units, 4 KiB) at LANE l; kChunks chunks are a SLICE (64 KiB), slice s holding the chunks 16 s .. 16 s + 15.  The terms (x, or
//   |x|^2) past the window's end are +0.0.  Then
//     1. inside a unit     adjacent pairs of elements, then adjacent pairs of those sums, ... (a unit holds 1 to 16 elements)
//     2. inside a slice    per lane, over its 16 chunks: chunks c and c ^ 1, then the pairs c and c ^ 2, c ^ 4, c ^ 8
//     3. across the lanes  l and l ^ 1, then l ^ 2, ... l ^ 128 (the last two steps join the four waves)
//     4. across the slices adjacent pairs of slice sums, then adjacent pairs of those, ...
//   and one division by N (and the square root) follows.  A sum with +0.0 is exact, so the levels that round are those at which
//   both halves hold an element: at most ceil(log2 N) on the way of any term.  A window that ends inside its first slice stops after
//   step 3; a longer one leaves a partial per slice, which a second kernel joins by step 4 -- the same tree either way, so the
//   position in a batch, the byte address, the number of windows in a launch and the path leave every bit of a result alone.
// A window of at most four chunks (16 KiB) is reduced by a wave alone, four windows to a workgroup and no barrier: the wave stands in
// for the four waves of the tree, lane l for the lanes l, l + 64, l + 128 and l + 192 (of a window of at most 64 units the lanes
// 64 .. 255 hold +0.0 and are left out).
// No atomics, no order of arrival, nothing kept in private memory.
#include "pcx_internal.hpp"
#include "unit_io.hpp"

namespace pcx {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;                         // lanes of the tree: four waves
constexpr int kChunks = 16;                           // chunks of a slice
constexpr int kChunkBytes = kThreads * 16;
constexpr int64_t kSliceBytes = (int64_t)kChunks * kChunkBytes;
constexpr int kLoads = 4;                             // units a lane has in flight
constexpr int kPartPerThread = 256;                   // partials a thread of the second kernel joins at most
constexpr size_t kMaxSlices = (size_t)kThreads * kPartPerThread;
constexpr unsigned kMaxGrid = 1u << 30;

static_assert(kChunks % kLoads == 0 && (kChunks & (kChunks - 1)) == 0, "a slice is a power of two of chunks, read kLoads at a time");

struct Acc {
    double re, im;
};
template <bool TWO>
__device__ __forceinline__ Acc join(const Acc &a, const Acc &b)
{
    Acc r;
    r.re = a.re + b.re;
    r.im = TWO ? a.im + b.im : 0.0;
    return r;
}

// lane l receives the value of lane l ^ O
template <int O>
__device__ __forceinline__ double lane_xor(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (O < 32) {                           // ds_swizzle, bit mode: and 0x1F, or 0, xor O inside each half of the wave
        lo = __builtin_amdgcn_ds_swizzle(lo, (O << 10) | 0x1F);
        hi = __builtin_amdgcn_ds_swizzle(hi, (O << 10) | 0x1F);
    } else {
        lo = __shfl_xor(lo, O, kWave);
        hi = __shfl_xor(hi, O, kWave);
    }
    return __hiloint2double(hi, lo);
}
template <bool TWO, int O>
__device__ __forceinline__ Acc wave_step(const Acc &a)
{
    Acc o;
    o.re = lane_xor<O>(a.re);
    o.im = TWO ? lane_xor<O>(a.im) : 0.0;
    return join<TWO>(a, o);
}
// step 3 inside a wave: every lane ends with the sum of the 64
template <bool TWO>
__device__ __forceinline__ Acc wave_sum(Acc a)
{
    a = wave_step<TWO, 1>(a);
    a = wave_step<TWO, 2>(a);
    a = wave_step<TWO, 4>(a);
    a = wave_step<TWO, 8>(a);
    a = wave_step<TWO, 16>(a);
    a = wave_step<TWO, 32>(a);
    return a;
}

// step 1: the terms of one unit (bytes past the window's end arrive as zeros: +0.0 in every type)
template <typename S, bool CPLX, int MODE>
__device__ __forceinline__ Acc unit_sum(const uint4 &v)
{
    constexpr bool TWO = CPLX && MODE == PCX_PROBE_MEAN;
    constexpr int NS = 16 / (int)sizeof(S), E = CPLX ? NS / 2 : NS;
    S s[NS];
    __builtin_memcpy(s, &v, 16);
    Acc t[E];
#pragma unroll
    for (int j = 0; j < E; j++) {
        if constexpr (CPLX) {
            const double re = (double)s[2 * j], im = (double)s[2 * j + 1];
            if constexpr (MODE == PCX_PROBE_MEAN) {
                t[j].re = re;
                t[j].im = im;
            } else {
                const double m = hypot(re, im);       // std::abs(std::complex<double>), SignalProbe.cpp:149
                t[j].re = m * m;
                t[j].im = 0.0;
            }
        } else {
            const double x = (double)s[j];
            t[j].re = MODE == PCX_PROBE_MEAN ? x : x * x;
            t[j].im = 0.0;
        }
    }
#pragma unroll
    for (int w = 1; w < E; w *= 2)
#pragma unroll
        for (int j = 0; j + w < E; j += 2 * w) t[j] = join<TWO>(t[j], t[j + w]);
    return t[0];
}

// step 2: the chunks c0 .. c0 + L - 1 of the slice at p, for lane l; nbytes: what the window has from p on.  Whole chunks past the
// window's end are skipped (the same for every lane): their sum is +0.0
template <typename S, bool CPLX, int MODE, int L>
__device__ __forceinline__ Acc chunk_sum(const unsigned char *p, int64_t nbytes, int c0, int l)
{
    constexpr bool TWO = CPLX && MODE == PCX_PROBE_MEAN;
    if constexpr (L <= kLoads) {
        uint4 v[L];
#pragma unroll
        for (int i = 0; i < L; i++) v[i] = load_unit(p, ((int64_t)(c0 + i) * kThreads + l) * 16, nbytes);
        Acc a[L];
#pragma unroll
        for (int i = 0; i < L; i++) a[i] = unit_sum<S, CPLX, MODE>(v[i]);
#pragma unroll
        for (int w = 1; w < L; w *= 2)
#pragma unroll
            for (int i = 0; i + w < L; i += 2 * w) a[i] = join<TWO>(a[i], a[i + w]);
        return a[0];
    } else {
        Acc zero;
        zero.re = zero.im = 0.0;
        if ((int64_t)c0 * kChunkBytes >= nbytes) return zero;
        const Acc a = chunk_sum<S, CPLX, MODE, L / 2>(p, nbytes, c0, l);
        const Acc b = chunk_sum<S, CPLX, MODE, L / 2>(p, nbytes, c0 + L / 2, l);
        return join<TWO>(a, b);
    }
}

// the division and the root (SignalProbe.cpp:152, :158); + 0.0: a sum of -0.0 terms is +0.0, as the reference's accumulator gives
template <bool TWO, int MODE>
__device__ __forceinline__ void finish(const Acc &a, int64_t N, double *out)
{
    const double d = (double)N;
    if constexpr (MODE == PCX_PROBE_RMS) {
        out[0] = sqrt((a.re + 0.0) / d);
        out[1] = 0.0;
    } else {
        out[0] = (a.re + 0.0) / d;
        out[1] = TWO ? (a.im + 0.0) / d : 0.0;
    }
}

// Windows w0 .. w0 + nwin - 1 of the stream (n elements, W to a window, the last window the remainder).
//   per_wave   a window has at most kLoads chunks: wave v of workgroup b reduces window w0 + 4 b + v and writes its result
//   else       workgroup b reduces slice b % ns of window w0 + b / ns; with ns == 1 it writes the result, else the slice's partial
template <typename S, bool CPLX, int MODE>
__global__ __launch_bounds__(kThreads) void probe_reduce_kernel(const unsigned char *__restrict__ in, int64_t n, int64_t W, int64_t w0, int64_t nwin,
                                                                int64_t ns, int per_wave, double *__restrict__ out)
{
    constexpr bool TWO = CPLX && MODE == PCX_PROBE_MEAN;
    constexpr int64_t ES = (int64_t)sizeof(S) * (CPLX ? 2 : 1);
    __shared__ double part[kThreads / kWave][2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;

    if (per_wave) {
        const int64_t wl = (int64_t)blockIdx.x * (kThreads / kWave) + wave;
        if (wl >= nwin) return;
        const int64_t e0 = (w0 + wl) * W, N = W < n - e0 ? W : n - e0, nbytes = N * ES;
        const unsigned char *p = in + e0 * ES;
        Acc r;
        if (nbytes <= (int64_t)kWave * 16) {          // at most 64 units: the lanes 64 .. 255 of the tree hold +0.0
            r = wave_sum<TWO>(chunk_sum<S, CPLX, MODE, 1>(p, nbytes, 0, lane));
        } else {                                      // the wave stands in for the four: lane l is the lanes l, l + 64, l + 128, l + 192
            Acc a[kThreads / kWave];
            if (nbytes <= kChunkBytes) {
#pragma unroll
                for (int v = 0; v < kThreads / kWave; v++) a[v] = chunk_sum<S, CPLX, MODE, 1>(p, nbytes, 0, lane + kWave * v);
            } else {
#pragma unroll
                for (int v = 0; v < kThreads / kWave; v++) a[v] = chunk_sum<S, CPLX, MODE, kLoads>(p, nbytes, 0, lane + kWave * v);
            }
#pragma unroll
            for (int v = 0; v < kThreads / kWave; v++) a[v] = wave_sum<TWO>(a[v]);
            r = join<TWO>(join<TWO>(a[0], a[1]), join<TWO>(a[2], a[3]));
        }
        if (lane == 0) finish<TWO, MODE>(r, N, out + 2 * (w0 + wl));
        return;
    }

    const int64_t wl = (int64_t)blockIdx.x / ns, s = (int64_t)blockIdx.x % ns;
    const int64_t e0 = (w0 + wl) * W, N = W < n - e0 ? W : n - e0;
    const int64_t b0 = s * kSliceBytes, left = N * ES - b0;             // (left <= 0: a slice past the remainder window's end)
    Acc a = chunk_sum<S, CPLX, MODE, kChunks>(in + e0 * ES + b0, left, 0, tid);
    a = wave_sum<TWO>(a);
    if (lane == 0) {
        part[wave][0] = a.re;
        part[wave][1] = a.im;
    }
    __syncthreads();
    if (tid != 0) return;
    Acc h[kThreads / kWave];
#pragma unroll
    for (int v = 0; v < kThreads / kWave; v++) {
        h[v].re = part[v][0];
        h[v].im = part[v][1];
    }
    const Acc r = join<TWO>(join<TWO>(h[0], h[1]), join<TWO>(h[2], h[3]));
    if (ns == 1) {
        finish<TWO, MODE>(r, N, out + 2 * (w0 + wl));
    } else {
        out[2 * blockIdx.x] = r.re;
        out[2 * blockIdx.x + 1] = r.im;
    }
}

// step 4 for one thread: the partials i0 .. i0 + L - 1 of ns
template <int L>
__device__ __forceinline__ Acc part_sum(const double *__restrict__ part, int64_t i0, int64_t ns)
{
    Acc zero;
    zero.re = zero.im = 0.0;
    if (i0 >= ns) return zero;
    if constexpr (L == 1) {
        Acc a;
        a.re = part[2 * i0];
        a.im = part[2 * i0 + 1];
        return a;
    } else {
        const Acc a = part_sum<L / 2>(part, i0, ns);
        const Acc b = part_sum<L / 2>(part, i0 + L / 2, ns);
        return join<true>(a, b);
    }
}

// workgroup b joins the ns partials of window w0 + b: thread t those from t L on, then the threads as the lanes of step 3 (adjacent
// pairs throughout: the result does not depend on L)
template <int MODE, int L>
__global__ __launch_bounds__(kThreads) void probe_join_kernel(const double *__restrict__ part, int64_t ns, int64_t n, int64_t W, int64_t w0,
                                                              double *__restrict__ out)
{
    __shared__ double wsum[kThreads / kWave][2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int64_t w = w0 + blockIdx.x, N = W < n - w * W ? W : n - w * W;
    Acc a = part_sum<L>(part + 2 * (int64_t)blockIdx.x * ns, (int64_t)tid * L, ns);
    a = wave_sum<true>(a);
    if (lane == 0) {
        wsum[wave][0] = a.re;
        wsum[wave][1] = a.im;
    }
    __syncthreads();
    if (tid != 0) return;
    Acc h[kThreads / kWave];
#pragma unroll
    for (int v = 0; v < kThreads / kWave; v++) {
        h[v].re = wsum[v][0];
        h[v].im = wsum[v][1];
    }
    const Acc r = join<true>(join<true>(h[0], h[1]), join<true>(h[2], h[3]));
    finish<true, MODE>(r, N, out + 2 * w);
}

// VALUE: the last element of every window, converted (SignalProbe.cpp:141)
template <typename S, bool CPLX>
__global__ __launch_bounds__(kThreads) void probe_value_kernel(const unsigned char *__restrict__ in, int64_t n, int64_t W, int64_t w0, int64_t nwin,
                                                               double *__restrict__ out)
{
    constexpr int64_t ES = (int64_t)sizeof(S) * (CPLX ? 2 : 1);
    const int64_t wl = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (wl >= nwin) return;
    const int64_t w = w0 + wl, last = ((w + 1) * W < n ? (w + 1) * W : n) - 1;
    S s[2] = {S(0), S(0)};
    __builtin_memcpy(s, in + last * ES, (size_t)ES);
    out[2 * w] = (double)s[0];
    out[2 * w + 1] = CPLX ? (double)s[1] : 0.0;
}

struct Job {
    const unsigned char *in;
    int64_t n, W, nwin;
    double *values, *part;
    hipStream_t st;
};

template <typename S, bool CPLX, int MODE>
int reduce(const Job &j)
{
    const int64_t es = (int64_t)sizeof(S) * (CPLX ? 2 : 1), wbytes = j.W * es;
    if (wbytes <= kSliceBytes) {                      // the small-window path: whole windows to a wave or a workgroup
        const int per_wave = wbytes <= (int64_t)kLoads * kChunkBytes;
        const int64_t per_block = per_wave ? kThreads / kWave : 1;
        for (int64_t w0 = 0; w0 < j.nwin;) {
            const int64_t take = std::min<int64_t>(j.nwin - w0, (int64_t)kMaxGrid * per_block);
            hipLaunchKernelGGL((probe_reduce_kernel<S, CPLX, MODE>), dim3((unsigned)((take + per_block - 1) / per_block)), dim3(kThreads), 0, j.st, j.in, j.n,
                               j.W, w0, take, (int64_t)1, per_wave, j.values);
            PCX_LAUNCH_CHECK();
            w0 += take;
        }
        return PCX_OK;
    }
    // the large-window path: a partial per slice, then the partials of a window joined in slice order
    const int64_t ns = (wbytes + kSliceBytes - 1) / kSliceBytes;
    if ((size_t)ns > kMaxSlices) {
        set_error("signal probe: a window of %lld elements exceeds %zu slices", (long long)j.W, kMaxSlices);
        return PCX_ERR_ARG;
    }
    const int64_t group = std::max<int64_t>(1, (int64_t)kMaxSlices / ns);
    for (int64_t w0 = 0; w0 < j.nwin; w0 += group) {
        const int64_t take = std::min(group, j.nwin - w0);
        hipLaunchKernelGGL((probe_reduce_kernel<S, CPLX, MODE>), dim3((unsigned)(take * ns)), dim3(kThreads), 0, j.st, j.in, j.n, j.W, w0, take, ns, 0, j.part);
        PCX_LAUNCH_CHECK();
        const dim3 g((unsigned)take), b(kThreads);
        const double *part = j.part;
        if (ns <= kThreads) hipLaunchKernelGGL((probe_join_kernel<MODE, 1>), g, b, 0, j.st, part, ns, j.n, j.W, w0, j.values);
        else if (ns <= 4 * kThreads) hipLaunchKernelGGL((probe_join_kernel<MODE, 4>), g, b, 0, j.st, part, ns, j.n, j.W, w0, j.values);
        else if (ns <= 16 * kThreads) hipLaunchKernelGGL((probe_join_kernel<MODE, 16>), g, b, 0, j.st, part, ns, j.n, j.W, w0, j.values);
        else if (ns <= 64 * kThreads) hipLaunchKernelGGL((probe_join_kernel<MODE, 64>), g, b, 0, j.st, part, ns, j.n, j.W, w0, j.values);
        else hipLaunchKernelGGL((probe_join_kernel<MODE, kPartPerThread>), g, b, 0, j.st, part, ns, j.n, j.W, w0, j.values);
        PCX_LAUNCH_CHECK();
    }
    return PCX_OK;
}

template <typename S, bool CPLX>
int value(const Job &j)
{
    for (int64_t w0 = 0; w0 < j.nwin;) {
        const int64_t take = std::min<int64_t>(j.nwin - w0, (int64_t)kMaxGrid * kThreads);
        hipLaunchKernelGGL((probe_value_kernel<S, CPLX>), dim3((unsigned)((take + kThreads - 1) / kThreads)), dim3(kThreads), 0, j.st, j.in, j.n, j.W, w0, take,
                           j.values);
        PCX_LAUNCH_CHECK();
        w0 += take;
    }
    return PCX_OK;
}

template <typename S, bool CPLX>
int by_mode(int mode, const Job &j)
{
    switch (mode) {
    case PCX_PROBE_VALUE: return value<S, CPLX>(j);
    case PCX_PROBE_RMS: return reduce<S, CPLX, PCX_PROBE_RMS>(j);
    case PCX_PROBE_MEAN: return reduce<S, CPLX, PCX_PROBE_MEAN>(j);
    }
    set_error("signal probe: unknown mode %d", mode);
    return PCX_ERR_ARG;
}

template <typename S>
int by_kind(bool cplx, int mode, const Job &j)
{
    return cplx ? by_mode<S, true>(mode, j) : by_mode<S, false>(mode, j);
}

}  // namespace

size_t probe_tile(int scalar, bool cplx) { return (size_t)kSliceBytes / ((size_t)scalar_bytes(scalar) * (cplx ? 2 : 1)); }
size_t probe_slice(int scalar, bool cplx) { return probe_tile(scalar, cplx); }
size_t probe_max_slices() { return kMaxSlices; }

int launch_probe_windows(int scalar, bool cplx, int mode, const void *in, size_t n, size_t W, double *values, double *part, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    if (W == 0) {
        set_error("signal probe: a window of 0 elements");
        return PCX_ERR_ARG;
    }
    Job j;
    j.in = static_cast<const unsigned char *>(in);
    j.n = (int64_t)n;
    j.W = (int64_t)std::min(W, n);                    // (one window: its length is what the tree depends on)
    j.nwin = (int64_t)((n + W - 1) / W);
    j.values = values;
    j.part = part;
    j.st = st;
    switch (scalar) {
    case PCX_F64: return by_kind<double>(cplx, mode, j);
    case PCX_F32: return by_kind<float>(cplx, mode, j);
    case PCX_I64: return by_kind<int64_t>(cplx, mode, j);
    case PCX_I32: return by_kind<int32_t>(cplx, mode, j);
    case PCX_I16: return by_kind<int16_t>(cplx, mode, j);
    case PCX_I8: return by_kind<int8_t>(cplx, mode, j);
    }
    set_error("signal probe: unsupported type (scalar %d)", scalar);
    return PCX_ERR_ARG;
}

}  // namespace pcx
