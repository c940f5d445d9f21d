// iir.hip -- /comms/iir_filter (filter/IIRFilter.cpp): y[n] = sum_{k=0..N} b_k x[n-k] - sum_{k=1..N} a_k y[n-k] in double, per
// component, narrowed to the stream type.  Two plans:
//   SCAN    stable filters (Schur-Cohn), the order padded to a bucket NB in {2, 4, 8, 16, 32}.  The state is s = (y[n], ..., y[n-NB+1])
//           and s' = M s + e1 v with the companion matrix M.  One call slice of at most 64 Mi samples runs as four launches:
//             tile    per 4096-sample tile: every thread's 16 samples from zero state, then a log-step scan of the threads' end
//                     states with M^16, M^32, ..., M^2048: the tile's zero-state end state z_t
//             carry   one workgroup: s_t = M^4096 s_{t-1} + z_t over the tiles from the carried state, runs of 64 tiles per thread
//                     and a log-step scan of the runs with powers of M^(64*4096): each tile's incoming state
//             apply   the tile again, the scan folded with the tile's incoming state: every thread's incoming state, then its
//                     16 outputs = the zero-state response + G16 . s, narrowed and stored through LDS
//             finish  the carried history := the last 32 inputs and outputs of the slice
//           Held to the bound of pcx_iir_get_plan, not to bits: it reassociates and fuses.
//   SERIAL  every other filter: one thread per component, the exact order N, the sequential loop of tests/iir_model.py operation by
//           operation (the tree builds with -ffp-contract=off): bit for bit the model.
// No workgroup waits for another, the state lives at fixed addresses, and every sample index is 64-bit.
#include <limits>
#include <type_traits>

#include "pcx_internal.hpp"

namespace pcx {
namespace {

constexpr int kNT = 256;              // threads per tile workgroup
constexpr int kS = 16;                // samples per thread
constexpr int kTile = kNT * kS;       // 4096
constexpr int kH = 32;                // halo slots in front of a tile (the largest order)
constexpr int kRun = 64;              // tiles per thread of the carry scan: kNT * kRun tiles = one slice
constexpr int kScanSteps = 8;         // log2(kNT)

template <typename T, int C>
struct Elem {
    T v[C];
};

// LDS slot of tile element e (e = -kH ... kTile-1): one pad element per 16, so that the threads' 16-element windows start in
// different banks
__host__ __device__ constexpr int slot(int e) { return (e + kH) + ((e + kH) >> 4); }
constexpr int kSlots = slot(kTile) + 1;

template <typename T>
__device__ inline T narrow(double y)
{
    if constexpr (std::is_same<T, double>::value) {
        return y;
    } else if constexpr (std::is_same<T, float>::value) {
        return (float)y;                                       // round to nearest
    } else {
        // truncate toward zero; beyond the range of T saturate, NaN -> 0
        if (!(y == y)) return 0;
        if constexpr (sizeof(T) == 8) {
            if (y >= 9223372036854775808.0) return std::numeric_limits<T>::max();
            if (y <= -9223372036854775808.0) return std::numeric_limits<T>::min();
        } else {
            if (y >= (double)std::numeric_limits<T>::max()) return std::numeric_limits<T>::max();
            if (y <= (double)std::numeric_limits<T>::min()) return std::numeric_limits<T>::min();
        }
        return (T)y;
    }
}

// table of a SCAN bucket (pcx_iir_api.hip iir_tables): b[0..NB], -a[0..NB], G16[16][NB], P[0..8] = M^(16 * 2^d) (P[8] = M^4096),
// Q[0..7] = M^(4096 * 64 * 2^d); matrices row-major NB x NB
template <int NB>
struct Tab {
    static constexpr int b = 0, na = NB + 1, G = 2 * (NB + 1), P = G + kS * NB, Q = P + 9 * NB * NB;
};

// E += P x
template <int NB>
__device__ inline void mv_acc(double (&E)[NB], const double *__restrict__ P, const double (&x)[NB])
{
#pragma unroll
    for (int r = 0; r < NB; r++) {
        double acc = E[r];
#pragma unroll
        for (int k = 0; k < NB; k++) acc = fma(P[r * NB + k], x[k], acc);
        E[r] = acc;
    }
}

// inclusive log-step scan over the workgroup's threads: E_i <- E_i + Pw[d] E_(i - 2^d); sc holds NB x kNT doubles.  On return sc
// holds the inclusive results.
template <int NB>
__device__ inline void wg_scan(double (&E)[NB], double *sc, const double *__restrict__ Pw)
{
    const int i = threadIdx.x;
#pragma unroll 1
    for (int d = 0; d < kScanSteps; d++) {
#pragma unroll
        for (int k = 0; k < NB; k++) sc[k * kNT + i] = E[k];
        __syncthreads();
        const int o = 1 << d;
        if (i >= o) {
            double Ep[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) Ep[k] = sc[k * kNT + i - o];
            mv_acc<NB>(E, Pw + (size_t)d * NB * NB, Ep);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NB; k++) sc[k * kNT + i] = E[k];
    __syncthreads();
}

// the tile [t0, t0 + 4096) and its 32-element halo into LDS, coalesced; elements past m are zero; the halo of tile 0 is the carried
// input history (xh[k] = x[-1-k])
template <typename T, int C>
__device__ inline void load_tile(Elem<T, C> *xs, const Elem<T, C> *__restrict__ in, int64_t t0, int64_t m, const Elem<T, C> *__restrict__ xh)
{
    for (int e = (int)threadIdx.x - kH; e < kTile; e += kNT) {
        const int64_t g = t0 + e;
        Elem<T, C> v;
        if (g < 0) v = xh[-1 - g];
        else if (g < m) v = in[g];
        else {
#pragma unroll
            for (int c = 0; c < C; c++) v.v[c] = 0;
        }
        xs[slot(e)] = v;
    }
    __syncthreads();
}

// the thread's 16 zero-state outputs of component c: v_j by the feedforward taps over the window, then the all-pole recurrence from
// zero, the terms that do not depend on y[j-1] first
template <typename T, int C, int NB>
__device__ inline void zero_state(double (&y)[kS], const Elem<T, C> *xs, int c, const double *__restrict__ tab)
{
    const int base = (int)threadIdx.x * kS - NB;
    double w[NB + kS];
#pragma unroll
    for (int q = 0; q < NB + kS; q++) w[q] = (double)xs[slot(base + q)].v[c];
    const double *b = tab + Tab<NB>::b, *na = tab + Tab<NB>::na;
#pragma unroll
    for (int j = 0; j < kS; j++) {
        double acc = b[NB] * w[j];
#pragma unroll
        for (int k = NB - 1; k >= 0; k--) acc = fma(b[k], w[j + NB - k], acc);
        y[j] = acc;
    }
#pragma unroll
    for (int j = 0; j < kS; j++) {
        double acc = y[j];
#pragma unroll
        for (int k = NB; k >= 2; k--)
            if (j - k >= 0) acc = fma(na[k], y[j - k], acc);
        if (j >= 1) acc = fma(na[1], y[j - 1], acc);
        y[j] = acc;
    }
}

template <int NB>
__device__ inline void end_state(double (&E)[NB], const double (&y)[kS])
{
#pragma unroll
    for (int k = 0; k < NB; k++) E[k] = k < kS ? y[kS - 1 - (k < kS ? k : 0)] : 0.0;
}

template <typename T, int C, int NB>
__global__ __launch_bounds__(kNT) void iir_tile_kernel(const Elem<T, C> *__restrict__ in, int64_t m, const Elem<T, C> *__restrict__ xh,
                                                        const double *__restrict__ tab, double *__restrict__ z)
{
    __shared__ Elem<T, C> xs[kSlots];
    __shared__ double sc[NB * kNT];
    const int64_t t = blockIdx.x;
    load_tile<T, C>(xs, in, t * kTile, m, xh);
#pragma unroll
    for (int c = 0; c < C; c++) {
        double y[kS], E[NB];
        zero_state<T, C, NB>(y, xs, c, tab);
        end_state<NB>(E, y);
        wg_scan<NB>(E, sc, tab + Tab<NB>::P);
        if (threadIdx.x == kNT - 1) {
#pragma unroll
            for (int k = 0; k < NB; k++) z[(t * C + c) * NB + k] = E[k];
        }
    }
}

template <typename T, int C, int NB>
__global__ __launch_bounds__(kNT) void iir_apply_kernel(const Elem<T, C> *__restrict__ in, Elem<T, C> *__restrict__ out, int64_t m,
                                                         const Elem<T, C> *__restrict__ xh, const double *__restrict__ tab,
                                                         const double *__restrict__ tin, double *__restrict__ ytail)
{
    __shared__ Elem<T, C> xs[kSlots];
    __shared__ double sc[NB * kNT];
    const int64_t t = blockIdx.x, t0 = t * kTile;
    const int i = threadIdx.x;
    load_tile<T, C>(xs, in, t0, m, xh);
    double yv[C][kS];
#pragma unroll
    for (int c = 0; c < C; c++) {
        double E[NB], s[NB];
        zero_state<T, C, NB>(yv[c], xs, c, tab);
        end_state<NB>(E, yv[c]);
#pragma unroll
        for (int k = 0; k < NB; k++) s[k] = tin[(t * C + c) * NB + k];
        if (i == 0) mv_acc<NB>(E, tab + Tab<NB>::P, s);          // thread 0 ends at M^16 s_in + e_0
        wg_scan<NB>(E, sc, tab + Tab<NB>::P);
        if (i > 0) {
#pragma unroll
            for (int k = 0; k < NB; k++) s[k] = sc[k * kNT + i - 1];
        }
        __syncthreads();                                         // (sc is reused by the next component)
        const double *G = tab + Tab<NB>::G;
#pragma unroll
        for (int j = 0; j < kS; j++) {
            double acc = yv[c][j];
#pragma unroll
            for (int k = 0; k < NB; k++) acc = fma(G[j * NB + k], s[k], acc);
            yv[c][j] = acc;
        }
    }
    // the last 32 outputs of the slice, unrounded, for the carried history
    const int64_t g0 = t0 + (int64_t)i * kS;
    if (g0 + kS > m - kH && g0 < m) {
#pragma unroll
        for (int j = 0; j < kS; j++) {
            const int64_t g = g0 + j;
            if (g >= m - kH && g < m) {
#pragma unroll
                for (int c = 0; c < C; c++) ytail[c * kH + (m - 1 - g)] = yv[c][j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kS; j++) {
        Elem<T, C> o;
#pragma unroll
        for (int c = 0; c < C; c++) o.v[c] = narrow<T>(yv[c][j]);
        xs[slot(i * kS + j)] = o;
    }
    __syncthreads();
    for (int e = i; e < kTile; e += kNT) {
        const int64_t g = t0 + e;
        if (g < m) out[g] = xs[slot(e)];
    }
}

// one workgroup: every tile's incoming state from the carried one; thread r owns tiles [64 r, 64 r + 64)
template <int C, int NB>
__global__ __launch_bounds__(kNT) void iir_carry_kernel(const double *__restrict__ z, int64_t nt, const double *__restrict__ ystate,
                                                        const double *__restrict__ tab, double *__restrict__ tin)
{
    __shared__ double sc[NB * kNT];
    const int r = threadIdx.x;
    const int64_t t0 = (int64_t)r * kRun, t1 = t0 + kRun < nt ? t0 + kRun : nt;
    const double *MT = tab + Tab<NB>::P + 8 * NB * NB;
#pragma unroll 1
    for (int c = 0; c < C; c++) {
        double a[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) a[k] = r == 0 ? ystate[c * kH + k] : 0.0;
#pragma unroll 1
        for (int64_t t = t0; t < t1; t++) {
            double n[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) n[k] = z[(t * C + c) * NB + k];
            mv_acc<NB>(n, MT, a);
#pragma unroll
            for (int k = 0; k < NB; k++) a[k] = n[k];
        }
        wg_scan<NB>(a, sc, tab + Tab<NB>::Q);
        if (r == 0) {
#pragma unroll
            for (int k = 0; k < NB; k++) a[k] = ystate[c * kH + k];
        } else {
#pragma unroll
            for (int k = 0; k < NB; k++) a[k] = sc[k * kNT + r - 1];
        }
        __syncthreads();
#pragma unroll 1
        for (int64_t t = t0; t < t1; t++) {
            double n[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) {
                tin[(t * C + c) * NB + k] = a[k];
                n[k] = z[(t * C + c) * NB + k];
            }
            mv_acc<NB>(n, MT, a);
#pragma unroll
            for (int k = 0; k < NB; k++) a[k] = n[k];
        }
    }
}

// the carried history after a SCAN slice of m samples: xh[k] = x[m-1-k], ystate[c][k] = y[m-1-k], k < 32, from the slice where it
// reaches back that far and from the history before it otherwise
template <typename T, int C>
__global__ __launch_bounds__(64) void iir_finish_kernel(const Elem<T, C> *__restrict__ in, int64_t m, Elem<T, C> *__restrict__ xh,
                                                        double *__restrict__ ystate, const double *__restrict__ ytail)
{
    const int k = threadIdx.x;
    Elem<T, C> nx;
    double ny[C];
    if (k < kH) {
        nx = k < m ? in[m - 1 - k] : xh[k - m];
#pragma unroll
        for (int c = 0; c < C; c++) ny[c] = k < m ? ytail[c * kH + k] : ystate[c * kH + k - m];
    }
    __syncthreads();
    if (k < kH) {
        xh[k] = nx;
#pragma unroll
        for (int c = 0; c < C; c++) ystate[c * kH + k] = ny[c];
    }
}

// SERIAL: thread c runs component c in the model's order, the last 64 inputs and outputs in LDS rings indexed by sample mod 64
template <typename T, int C>
__global__ __launch_bounds__(64) void iir_serial_kernel(const Elem<T, C> *__restrict__ in, Elem<T, C> *__restrict__ out, int64_t m,
                                                        Elem<T, C> *__restrict__ xh, double *__restrict__ ystate,
                                                        const double *__restrict__ coef, int N)
{
    __shared__ T xr[C][64];
    __shared__ double yr[C][64];
    const int c = threadIdx.x;
    if (c >= C) return;
    for (int k = 0; k < kH; k++) {
        xr[c][(63 - k)] = xh[k].v[c];                 // x[-1-k] at (-1-k) mod 64
        yr[c][(63 - k)] = ystate[c * kH + k];
    }
    const double *b = coef, *a = coef + N + 1;
    for (int64_t n = 0; n < m; n++) {
        const int p = (int)(n & 63);
        xr[c][p] = in[n].v[c];
        double v = b[0] * (double)xr[c][p];
        for (int k = 1; k <= N; k++) v = v + b[k] * (double)xr[c][(p - k) & 63];
        double y = v;
        if (N >= 1) {
            double w = a[1] * yr[c][(p - 1) & 63];
            for (int k = 2; k <= N; k++) w = w + a[k] * yr[c][(p - k) & 63];
            y = v - w;
        }
        yr[c][p] = y;
        out[n].v[c] = narrow<T>(y);
    }
    const int p = (int)(m & 63);
    for (int k = 0; k < kH; k++) {
        xh[k].v[c] = xr[c][(p - 1 - k) & 63];
        ystate[c * kH + k] = yr[c][(p - 1 - k) & 63];
    }
}

template <typename T, int C, int NB>
int scan_t(const IirShape &p, const void *in, void *out, size_t m, void *xh, double *ystate, const double *tab, double *z, double *tin,
           double *ytail, hipStream_t st)
{
    using E = Elem<T, C>;
    const int64_t nt = (int64_t)((m + kTile - 1) / kTile);
    hipLaunchKernelGGL((iir_tile_kernel<T, C, NB>), dim3((unsigned)nt), dim3(kNT), 0, st, (const E *)in, (int64_t)m, (const E *)xh, tab, z);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((iir_carry_kernel<C, NB>), dim3(1), dim3(kNT), 0, st, (const double *)z, nt, (const double *)ystate, tab, tin);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((iir_apply_kernel<T, C, NB>), dim3((unsigned)nt), dim3(kNT), 0, st, (const E *)in, (E *)out, (int64_t)m,
                       (const E *)xh, tab, (const double *)tin, ytail);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((iir_finish_kernel<T, C>), dim3(1), dim3(64), 0, st, (const E *)in, (int64_t)m, (E *)xh, ystate, (const double *)ytail);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

template <typename T, int C>
int slice_t(const IirShape &p, const void *in, void *out, size_t m, void *xh, double *ystate, const double *tab, const double *coef,
            double *z, double *tin, double *ytail, hipStream_t st)
{
    if (p.plan == PCX_IIR_SERIAL) {
        using E = Elem<T, C>;
        hipLaunchKernelGGL((iir_serial_kernel<T, C>), dim3(1), dim3(64), 0, st, (const E *)in, (E *)out, (int64_t)m, (E *)xh, ystate, coef, p.N);
        PCX_LAUNCH_CHECK();
        return PCX_OK;
    }
    switch (p.NB) {
    case 2: return scan_t<T, C, 2>(p, in, out, m, xh, ystate, tab, z, tin, ytail, st);
    case 4: return scan_t<T, C, 4>(p, in, out, m, xh, ystate, tab, z, tin, ytail, st);
    case 8: return scan_t<T, C, 8>(p, in, out, m, xh, ystate, tab, z, tin, ytail, st);
    case 16: return scan_t<T, C, 16>(p, in, out, m, xh, ystate, tab, z, tin, ytail, st);
    case 32: return scan_t<T, C, 32>(p, in, out, m, xh, ystate, tab, z, tin, ytail, st);
    }
    set_error("iir_filter: no SCAN bucket for order %d", p.NB);
    return PCX_ERR_ARG;
}

}  // namespace

size_t iir_slice() { return (size_t)kRun * kNT * kTile; }
size_t iir_tile() { return kTile; }
int iir_history() { return kH; }

int launch_iir_slice(const IirShape &p, const void *in, void *out, size_t m, void *xh, double *ystate, const double *tab, const double *coef,
                     double *z, double *tin, double *ytail, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    switch (p.scalar * 2 + (p.cplx ? 1 : 0)) {
    case PCX_F64 * 2: return slice_t<double, 1>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_F64 * 2 + 1: return slice_t<double, 2>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_F32 * 2: return slice_t<float, 1>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_F32 * 2 + 1: return slice_t<float, 2>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I64 * 2: return slice_t<int64_t, 1>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I64 * 2 + 1: return slice_t<int64_t, 2>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I32 * 2: return slice_t<int32_t, 1>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I32 * 2 + 1: return slice_t<int32_t, 2>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I16 * 2: return slice_t<int16_t, 1>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I16 * 2 + 1: return slice_t<int16_t, 2>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I8 * 2: return slice_t<int8_t, 1>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    case PCX_I8 * 2 + 1: return slice_t<int8_t, 2>(p, in, out, m, xh, ystate, tab, coef, z, tin, ytail, st);
    }
    set_error("iir_filter: unsupported type (scalar %d)", p.scalar);
    return PCX_ERR_ARG;
}

}  // namespace pcx
