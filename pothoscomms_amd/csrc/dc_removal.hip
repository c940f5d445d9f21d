// dc_removal.hip -- /comms/dc_removal (filter/DCRemoval.cpp + filter/MovingAverage.hpp): C cascaded moving averages of depth D,
// out[n] = x[n-D+1] - y_C[n].
//
// A stage's accumulator is the running sum of the increments a0[n] = x[n] - x[n-D], i.e. a prefix sum, and a prefix sum in ring
// arithmetic is associative.  Two paths:
//   fused   the types whose accumulator telescopes to the window sum of the last D stage inputs (floats, held to exact arithmetic;
//           int8, int16, int64, complex_int64): one launch, every workgroup owns a tile of outputs, reads its input plus a halo of
//           H = C*h samples (h = D-1, D for int8) and runs all C stages out of one LDS prefix scan each.  No workgroup waits for
//           another.  Carried state: the last H input samples.
//   staged  the others (complex_int8/16/32 and int32 narrow the increment to the element type, so the running sum carries a wrap
//           count back to the last reset) and every type whose halo exceeds half a tile (2048 samples): per stage, reduce the increments per
//           tile, scan the tile sums in one workgroup from the carried accumulator, apply.  Carried state per stage: hist (D
//           samples) and the accumulator, exactly as the reference carries them.
// Every sample index is 64-bit.  The arithmetic of one stage, component by component (tests/dcr_model.py restates it):
//   inc   complex<T> or int32/int64: the difference narrowed to T; int8/int16: exact (promoted to int); floats: in double
//   b0    int8: int16(accumulator before the step) + a0, not wrapped; other integers: the accumulator wrapped to Acc
//   y     T(b0 / Acc(D)); complex integers: libstdc++'s generic division by complex<Acc>(D, 0), numerators and norm in Acc
#include <algorithm>

#include "pcx_internal.hpp"

namespace pcx {
namespace {

constexpr int kNT = 256;                 // threads per workgroup
constexpr int kK = 16;                   // consecutive samples per thread
constexpr int kTile = kNT * kK;          // samples per workgroup (fused: halo + outputs)
constexpr int kPad = kTile + kTile / 16; // LDS slots per component: one pad slot per 16 (the per-thread rows hit distinct banks)

__device__ inline int pad(int j) { return j + (j >> 4); }

__device__ inline int64_t wrapb(int64_t v, int bits)
{
    if (bits >= 64) return v;
    const int s = 64 - bits;
    return (int64_t)((uint64_t)v << s) >> s;
}
__device__ inline int64_t radd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ inline int64_t rsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
__device__ inline int64_t rmul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }
__device__ inline double radd(double a, double b) { return a + b; }
__device__ inline double rsub(double a, double b) { return a - b; }

template <typename T> struct Scalar;
template <> struct Scalar<double> { using R = double; static constexpr int tbits = 64, abits = 0; };
template <> struct Scalar<float> { using R = double; static constexpr int tbits = 32, abits = 0; };
template <> struct Scalar<int64_t> { using R = int64_t; static constexpr int tbits = 64, abits = 64; };
template <> struct Scalar<int32_t> { using R = int64_t; static constexpr int tbits = 32, abits = 64; };
template <> struct Scalar<int16_t> { using R = int64_t; static constexpr int tbits = 16, abits = 32; };
template <> struct Scalar<int8_t> { using R = int64_t; static constexpr int tbits = 8, abits = 16; };

template <typename T, bool CPLX>
struct Dcr {
    using S = Scalar<T>;
    using R = typename S::R;
    static constexpr int NC = CPLX ? 2 : 1;
    static constexpr bool FLOAT = S::abits == 0;
    static constexpr bool INT8_REAL = !CPLX && S::tbits == 8;

    __device__ static R inc(T u, T ud)
    {
        if constexpr (FLOAT) return (R)u - (R)ud;
        else if constexpr (CPLX || S::tbits >= 32) return wrapb(rsub((int64_t)u, (int64_t)ud), S::tbits);
        else return (int64_t)u - (int64_t)ud;
    }
    // the value the stage divides, from the running sum after the step (sum) and the step's increment (a)
    __device__ static R b0_of(R sum, R a)
    {
        if constexpr (FLOAT) return sum;
        else if constexpr (INT8_REAL) return wrapb(rsub(sum, a), 16) + a;
        else return wrapb(sum, S::abits);
    }
    __device__ static T y_of(R b0, int comp, int64_t D, int64_t dacc, int64_t nrm)
    {
        if constexpr (FLOAT) return (T)(b0 / (double)D);
        else if constexpr (!CPLX) return (T)(b0 / dacc);
        else {
            // re = Acc(re*D + im*0) / norm; im = (im*D - re*0) / norm, the numerator an int (not narrowed) when Acc is int16
            const int64_t p = rmul(b0, dacc);
            const int64_t num = (comp == 1 && S::abits == 16) ? p : wrapb(p, S::abits);
            return (T)wrapb(num / nrm, S::abits);
        }
    }
    __device__ static T out_of(T front, T y)
    {
        if constexpr (FLOAT) return front - y;
        else return (T)rsub((int64_t)front, (int64_t)y);
    }
};

// exclusive scan of one value per thread across the workgroup; *total = the sum of all
template <typename R>
__device__ inline R block_exclusive(R v, R *wave_tot, R *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    R s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const R t = __shfl_up(s, o, 64);
        if (lane >= o) s = radd(s, t);
    }
    if (lane == 63) wave_tot[wave] = s;
    __syncthreads();
    R before = R(0), all = R(0);
#pragma unroll
    for (int w = 0; w < kNT / 64; w++) {
        if (w < wave) before = radd(before, wave_tot[w]);
        all = radd(all, wave_tot[w]);
    }
    __syncthreads();
    *total = all;
    return radd(before, rsub(s, v));
}

// ---------------------------------------------------------------- fused path
// Tile of workgroup b: outputs [t0, t0 + kTile - H), t0 = b * (kTile - H); LDS position j holds stream index t0 - H + j.  Stage c
// (1-based) is exact at positions j >= c*h; the positions below feed nothing that is kept.
template <typename T, bool CPLX>
__global__ __launch_bounds__(kNT) void dcr_fused_kernel(const T *__restrict__ in, T *__restrict__ out, int64_t n,
                                                         const T *__restrict__ hx, int H, int D, int C, int64_t dacc, int64_t nrm)
{
    using Q = Dcr<T, CPLX>;
    using R = typename Q::R;
    constexpr int NC = Q::NC;
    __shared__ R P[NC][kPad];
    __shared__ R wave_tot[kNT / 64];
    __shared__ R tile_ref[NC];
    const int tid = threadIdx.x;
    const int64_t L = kTile - H;
    const int64_t t0 = (int64_t)blockIdx.x * L;
    const int64_t base = t0 - H;
    const int jref = (int)(n - 1 - base < kTile - 1 ? n - 1 - base : kTile - 1);    // the tile's last output position
    // stream sample i, component c: the carried samples in front of the call, zeros past its end
    auto load = [&](int64_t i, int c) -> T {
        if (i < 0) return hx[(size_t)(H + i) * NC + c];
        if (i < n) return in[(size_t)i * NC + c];
        return T(0);
    };
    for (int r = 0; r < kK; r++) {
        const int j = r * kNT + tid;
        for (int c = 0; c < NC; c++) P[c][pad(j)] = (R)load(base + j, c);
    }
    __syncthreads();
    R v[NC][kK];
    for (int c = 0; c < NC; c++)
        for (int i = 0; i < kK; i++) v[c][i] = P[c][pad(tid * kK + i)];
    auto Pat = [&](int c, int k) -> R { return k < 0 ? R(0) : P[c][pad(k)]; };
    for (int stage = 0; stage < C; stage++) {
        // floats: the prefix is taken of the samples minus the stage input at the tile's last output (past the start-up ramp of
        // every stage: H <= 2048 <= kTile - 1 - H), so that the rounding of P[j] - P[j-D] scales with the signal around that level
        // and not with a DC offset times the tile length
        R ref[NC];
        for (int c = 0; c < NC; c++) ref[c] = R(0);
        if constexpr (Q::FLOAT) {
            for (int c = 0; c < NC; c++)
                for (int i = 0; i < kK; i++)
                    if (tid * kK + i == jref) tile_ref[c] = v[c][i];
            __syncthreads();
            for (int c = 0; c < NC; c++) ref[c] = tile_ref[c];
        }
        for (int c = 0; c < NC; c++) {
            R acc = R(0), p[kK];
            for (int i = 0; i < kK; i++) { acc = radd(acc, rsub(v[c][i], ref[c])); p[i] = acc; }
            R tot;
            const R off = block_exclusive(acc, wave_tot, &tot);     // (its barriers also order the reads of the previous stage)
            for (int i = 0; i < kK; i++) P[c][pad(tid * kK + i)] = radd(off, p[i]);
        }
        __syncthreads();
        for (int c = 0; c < NC; c++) {
            for (int i = 0; i < kK; i++) {
                const int j = tid * kK + i;
                R sum = rsub(Pat(c, j), Pat(c, j - D));
                if constexpr (Q::FLOAT) sum += (R)D * ref[c];
                R a = R(0);
                if constexpr (Q::INT8_REAL) a = rsub(v[c][i], rsub(Pat(c, j - D), Pat(c, j - D - 1)));
                v[c][i] = (R)Q::y_of(Q::b0_of(sum, a), c, D, dacc, nrm);
            }
        }
    }
    __syncthreads();
    for (int c = 0; c < NC; c++)
        for (int i = 0; i < kK; i++) P[c][pad(tid * kK + i)] = v[c][i];
    __syncthreads();
    for (int r = 0; r < kK; r++) {
        const int j = r * kNT + tid;
        const int64_t t = base + j;
        if (j < H || t >= n) continue;
        for (int c = 0; c < NC; c++) out[(size_t)t * NC + c] = Q::out_of(load(t - D + 1, c), (T)P[c][pad(j)]);
    }
}

// ---------------------------------------------------------------- staged path (one stage of one chunk of m samples)
// u: the stage's input; hist: its D previous inputs (the reference's RingDeque, oldest first)
template <typename T, bool CPLX>
__device__ inline T stage_in(const T *u, const T *hist, int64_t k, int D, int c)
{
    constexpr int NC = CPLX ? 2 : 1;
    return k >= 0 ? u[(size_t)k * NC + c] : hist[(size_t)(D + k) * NC + c];
}

template <typename T, bool CPLX>
__global__ __launch_bounds__(kNT) void dcr_reduce_kernel(const T *__restrict__ u, int64_t m, const T *__restrict__ hist, int D,
                                                          typename Dcr<T, CPLX>::R *__restrict__ tsum)
{
    using Q = Dcr<T, CPLX>;
    using R = typename Q::R;
    __shared__ R wave_tot[kNT / 64];
    const int64_t k0 = (int64_t)blockIdx.x * kTile;
    for (int c = 0; c < Q::NC; c++) {
        R s = R(0);
        for (int r = 0; r < kK; r++) {
            const int64_t k = k0 + r * kNT + threadIdx.x;
            if (k < m) s = radd(s, Q::inc(stage_in<T, CPLX>(u, hist, k, D, c), stage_in<T, CPLX>(u, hist, k - D, D, c)));
        }
        R tot;
        (void)block_exclusive(s, wave_tot, &tot);
        if (threadIdx.x == 0) tsum[(size_t)blockIdx.x * Q::NC + c] = tot;
    }
}

// one workgroup: tile sums -> tile offsets (in place), from the carried accumulator b1, which then moves past the chunk
template <typename T, bool CPLX>
__global__ __launch_bounds__(kNT) void dcr_scan_kernel(typename Dcr<T, CPLX>::R *__restrict__ tsum, int64_t ntiles,
                                                        typename Dcr<T, CPLX>::R *__restrict__ b1)
{
    using Q = Dcr<T, CPLX>;
    using R = typename Q::R;
    __shared__ R wave_tot[kNT / 64];
    for (int c = 0; c < Q::NC; c++) {
        R carry = b1[c];
        for (int64_t b = 0; b < ntiles; b += kNT) {
            const int64_t i = b + threadIdx.x;
            const R v = i < ntiles ? tsum[(size_t)i * Q::NC + c] : R(0);
            R tot;
            const R ex = block_exclusive(v, wave_tot, &tot);
            if (i < ntiles) tsum[(size_t)i * Q::NC + c] = radd(carry, ex);
            carry = radd(carry, tot);
        }
        __syncthreads();
        if (threadIdx.x == 0) b1[c] = carry;
    }
}

// y = the stage's outputs; the last stage writes out = x[k-D+1] - y instead (x, hist0: the cascade's input and its history)
template <typename T, bool CPLX>
__global__ __launch_bounds__(kNT) void dcr_apply_kernel(const T *__restrict__ u, int64_t m, const T *__restrict__ hist, int D,
                                                         const typename Dcr<T, CPLX>::R *__restrict__ toff, T *__restrict__ y,
                                                         const T *__restrict__ x, const T *__restrict__ hist0, int last,
                                                         int64_t dacc, int64_t nrm)
{
    using Q = Dcr<T, CPLX>;
    using R = typename Q::R;
    constexpr int NC = Q::NC;
    __shared__ R wave_tot[kNT / 64];
    const int64_t k0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kK;
    for (int c = 0; c < NC; c++) {
        R a[kK], p[kK], acc = R(0);
        for (int i = 0; i < kK; i++) {
            const int64_t k = k0 + i;
            a[i] = k < m ? Q::inc(stage_in<T, CPLX>(u, hist, k, D, c), stage_in<T, CPLX>(u, hist, k - D, D, c)) : R(0);
            acc = radd(acc, a[i]);
            p[i] = acc;
        }
        R tot;
        const R off = radd(toff[(size_t)blockIdx.x * NC + c], block_exclusive(acc, wave_tot, &tot));
        for (int i = 0; i < kK; i++) {
            const int64_t k = k0 + i;
            if (k >= m) break;
            const T yv = Q::y_of(Q::b0_of(radd(off, p[i]), a[i]), c, D, dacc, nrm);
            if (last) y[(size_t)k * NC + c] = Q::out_of(stage_in<T, CPLX>(x, hist0, k - D + 1, D, c), yv);
            else y[(size_t)k * NC + c] = yv;
        }
    }
}

// the last `len` bytes of (old[0..len) ++ u[0..m)) -> tmp, then back into old (two launches: no in-place hazard, and the state
// keeps its address, so a captured call replays against it)
__global__ void dcr_shift_kernel(const unsigned char *__restrict__ old, const unsigned char *__restrict__ u, size_t m, size_t len,
                                 unsigned char *__restrict__ tmp)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
        tmp[i] = (m + i < len) ? old[m + i] : u[m + i - len];
}
__global__ void dcr_copy_kernel(unsigned char *__restrict__ dst, const unsigned char *__restrict__ src, size_t len)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

template <typename T, bool CPLX>
int fused_t(const DcrShape &p, const void *in, void *out, size_t n, const void *hx, hipStream_t st)
{
    const int64_t L = kTile - p.H;
    const size_t grid = (n + (size_t)L - 1) / (size_t)L;
    if (grid > 0x7fffffffu) { set_error("dc_removal: %zu samples in one call", n); return PCX_ERR_ARG; }
    hipLaunchKernelGGL((dcr_fused_kernel<T, CPLX>), dim3((unsigned)grid), dim3(kNT), 0, st, (const T *)in, (T *)out, (int64_t)n,
                       (const T *)hx, (int)p.H, (int)p.D, p.C, p.dacc, p.nrm);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

template <typename T, bool CPLX>
int stage_t(const DcrShape &p, const void *u, size_t m, const void *hist, void *tsum, void *b1, void *y, const void *x,
            const void *hist0, bool last, hipStream_t st)
{
    using R = typename Dcr<T, CPLX>::R;
    const size_t tiles = (m + kTile - 1) / kTile;
    hipLaunchKernelGGL((dcr_reduce_kernel<T, CPLX>), dim3((unsigned)tiles), dim3(kNT), 0, st, (const T *)u, (int64_t)m, (const T *)hist,
                       (int)p.D, (R *)tsum);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((dcr_scan_kernel<T, CPLX>), dim3(1), dim3(kNT), 0, st, (R *)tsum, (int64_t)tiles, (R *)b1);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((dcr_apply_kernel<T, CPLX>), dim3((unsigned)tiles), dim3(kNT), 0, st, (const T *)u, (int64_t)m, (const T *)hist,
                       (int)p.D, (const R *)tsum, (T *)y, (const T *)x, (const T *)hist0, last ? 1 : 0, p.dacc, p.nrm);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace

#define PCX_DCR_DISPATCH(fn, ...)                                                                   \
    switch (p.scalar * 2 + (p.cplx ? 1 : 0)) {                                                     \
    case PCX_F64 * 2: return fn<double, false>(__VA_ARGS__);                                       \
    case PCX_F64 * 2 + 1: return fn<double, true>(__VA_ARGS__);                                    \
    case PCX_F32 * 2: return fn<float, false>(__VA_ARGS__);                                        \
    case PCX_F32 * 2 + 1: return fn<float, true>(__VA_ARGS__);                                     \
    case PCX_I64 * 2: return fn<int64_t, false>(__VA_ARGS__);                                      \
    case PCX_I64 * 2 + 1: return fn<int64_t, true>(__VA_ARGS__);                                   \
    case PCX_I32 * 2: return fn<int32_t, false>(__VA_ARGS__);                                      \
    case PCX_I32 * 2 + 1: return fn<int32_t, true>(__VA_ARGS__);                                   \
    case PCX_I16 * 2: return fn<int16_t, false>(__VA_ARGS__);                                      \
    case PCX_I16 * 2 + 1: return fn<int16_t, true>(__VA_ARGS__);                                   \
    case PCX_I8 * 2: return fn<int8_t, false>(__VA_ARGS__);                                        \
    case PCX_I8 * 2 + 1: return fn<int8_t, true>(__VA_ARGS__);                                     \
    }                                                                                              \
    set_error("dc_removal: unsupported type (scalar %d)", p.scalar);                               \
    return PCX_ERR_ARG;

bool dcr_telescopes(int scalar, bool cplx)
{
    if (scalar == PCX_F64 || scalar == PCX_F32 || scalar == PCX_I64) return true;
    return !cplx && (scalar == PCX_I16 || scalar == PCX_I8);
}
int64_t dcr_fused_halo_max() { return kTile / 2; }

int launch_dcr_fused(const DcrShape &p, const void *in, void *out, size_t n, const void *hx, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    PCX_DCR_DISPATCH(fused_t, p, in, out, n, hx, st)
}
int launch_dcr_stage(const DcrShape &p, const void *u, size_t m, const void *hist, void *tsum, void *b1, void *y, const void *x,
                     const void *hist0, bool last, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    PCX_DCR_DISPATCH(stage_t, p, u, m, hist, tsum, b1, y, x, hist0, last, st)
}
size_t dcr_tile() { return kTile; }
int launch_dcr_shift(void *state, const void *u, size_t m_bytes, size_t len_bytes, void *tmp, hipStream_t st)
{
    if (len_bytes == 0 || m_bytes == 0) return PCX_OK;
    const unsigned grid = (unsigned)std::min<size_t>((len_bytes + 255) / 256, 1024);
    hipLaunchKernelGGL(dcr_shift_kernel, dim3(grid), dim3(256), 0, st, (const unsigned char *)state, (const unsigned char *)u, m_bytes,
                       len_bytes, (unsigned char *)tmp);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL(dcr_copy_kernel, dim3(grid), dim3(256), 0, st, (unsigned char *)state, (const unsigned char *)tmp, len_bytes);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace pcx
