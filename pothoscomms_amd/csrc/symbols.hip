// symbols.hip -- the four blocks that join the bit side to the sample side:
//   /comms/symbol_mapper          digital/SymbolMapper.cpp:89-91          out[i] = map[in[i] & mask]
//   /comms/symbol_slicer          digital/SymbolSlicer.cpp:43-52, 88-98   out[i] = the first map entry with the strictly smallest float distance
//   /comms/differential_encoder   digital/DifferentialEncoder.cpp:59-63   last = (in[i] + last + symbols) % symbols
//   /comms/differential_decoder   digital/DifferentialDecoder.cpp:59-64   out[i] = (in[i] - in[i-1] + symbols) % symbols
// Every output byte and element equals the reference's loop.
//   mapper   the handle expands the map to all 256 byte values (tab[b] = map[b & mask]); a workgroup holds the table in LDS, stages a
//            tile of 4096 input bytes (16 per lane) and writes the outputs as 16-byte units, lanes side by side.
//   slicer   the map lies in LDS in the type the reference subtracts in (int for int8 / int16 / int32, long for int64, float, double),
//            every lane reads the same entry (a broadcast).  A lane owns 4 consecutive samples (8 of 2 bytes, 16 of 1 byte), loads them
//            16 bytes at a time and stores their bytes as one dword or wider.  The distance is one rounding per step: the difference
//            in the promoted type, its conversion to float, and for complex types two separately rounded products and one sum (the
//            functions switch contraction off for themselves).  Integer differences that leave the signed type wrap (the reference is
//            undefined there).  Maps beyond slicer_max_onchip() entries are read from global memory by the same code.
//   decoder  a workgroup loads its tile whole, every lane leaves its last byte in LDS for its neighbour, the byte in front of the tile
//            comes from a halo pass that ran before (so out may be in itself); the same unsigned 32-bit arithmetic for every symbols.
//   encoder  SCAN (the step equals (in + last) mod m, m = min(symbols, 256), for all 65536 byte pairs -- checked by the handle):
//            out[i] = (carry + in[0] + ... + in[i]) mod m as tile sums, a one-workgroup carry over at most 16384 tiles and an apply pass
//            (per-lane run sums, a wave scan, the waves joined in LDS).  Sums are 32-bit words reduced mod m where needed: a tile sums to
//            at most 255 * 4096 < 2^21.  SERIAL: one thread runs the reference's loop as written, for every other symbols.
// The 16-byte loads and stores go through memcpy from byte pointers, so they hold at any alignment of either pointer (gfx950 takes
// unaligned global accesses at full width); only a tile or a group that is not whole goes element by element.
// No workgroup waits for another, the carried byte lives at a fixed address, every element index is 64-bit.
#include "pcx_internal.hpp"

namespace pcx {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kTile = kBlock * 16;              // bytes per workgroup of the mapper and the coders
constexpr int kSliceLog = 26;                   // elements per call slice
constexpr int kCarryThreads = 1024;
constexpr int kCarryRun = (1 << kSliceLog) / kTile / kCarryThreads;     // tiles per thread of the carry: 16
constexpr int kMaxOnChip = 1024;                // slicer: map entries held in LDS (16 KiB of complex double)

static_assert(kCarryRun * kCarryThreads * kTile == (1 << kSliceLog), "the carry covers one slice");

// ---------------------------------------------------------------- 16 bytes per lane
// the lane's bytes [i0, i0 + 16) of `in` as four words (byte q = bits 8 (q % 4) of word q / 4); bytes at and past n read as 0
__device__ inline int load16(const unsigned char *in, int64_t i0, int64_t n, uint32_t (&w)[4])
{
    const int64_t left = n - i0;
    const int cnt = left <= 0 ? 0 : left >= 16 ? 16 : (int)left;
    if (cnt == 16) {
        __builtin_memcpy(w, in + i0, 16);
        return cnt;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (int q = 0; q < 16; q++)
        if (q < cnt) w[q >> 2] |= (uint32_t)in[i0 + q] << (8 * (q & 3));
    return cnt;
}
__device__ inline void store16(unsigned char *out, int64_t i0, int cnt, const uint32_t (&w)[4])
{
    if (cnt == 16) {
        __builtin_memcpy(out + i0, w, 16);
        return;
    }
#pragma unroll
    for (int q = 0; q < 16; q++)
        if (q < cnt) out[i0 + q] = (unsigned char)(w[q >> 2] >> (8 * (q & 3)));
}
__device__ inline uint32_t byte_sum(uint32_t w)
{
    const uint32_t p = (w & 0x00FF00FFu) + ((w >> 8) & 0x00FF00FFu);
    return (p & 0xFFFFu) + (p >> 16);
}

// v mod m for v < 2^21: the float quotient is off by at most one either way, and is put right
__device__ inline uint32_t mod_small(uint32_t v, uint32_t m, float rcp)
{
    const uint32_t q = (uint32_t)((float)v * rcp);
    int32_t r = (int32_t)(v - q * m);
    if (r < 0) r += (int32_t)m;
    if ((uint32_t)r >= m) r -= (int32_t)m;
    return (uint32_t)r;
}

// ---------------------------------------------------------------- mapper
template <int ES> struct ElemWord;
template <> struct ElemWord<1> { typedef uint8_t type; };
template <> struct ElemWord<2> { typedef uint16_t type; };
template <> struct ElemWord<4> { typedef uint32_t type; };
template <> struct ElemWord<8> { typedef uint2 type; };
template <> struct ElemWord<16> { typedef uint4 type; };

// SB: bytes of a scalar, WPE: scalars per element.  tab: 256 elements, entry b = map[b & mask]
template <int SB, int WPE>
__global__ __launch_bounds__(kBlock) void sym_map_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, int64_t n,
                                                          const unsigned char *__restrict__ tab)
{
    constexpr int ES = SB * WPE, EPU = 16 / ES;          // elements per 16-byte output unit
    typedef typename ElemWord<ES>::type E;
    typedef typename ElemWord<SB>::type S;
    __shared__ uint4 tabs[256 * ES / 16];
    __shared__ uint4 stage[kBlock];
    for (int i = threadIdx.x; i < 256 * ES / 16; i += kBlock) tabs[i] = reinterpret_cast<const uint4 *>(tab)[i];
    __syncthreads();
    const unsigned char *sb = reinterpret_cast<const unsigned char *>(stage);
    const int64_t ntiles = (n + kTile - 1) / kTile;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t g0 = t * kTile;
        if (g0 + kTile <= n) {
            uint4 s;
            __builtin_memcpy(&s, in + g0 + 16 * (int64_t)threadIdx.x, 16);
            stage[threadIdx.x] = s;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ES; k++) {
                const int u = k * kBlock + threadIdx.x;      // the 16-byte unit of the tile's output
                E o[EPU];
#pragma unroll
                for (int q = 0; q < EPU; q++) o[q] = reinterpret_cast<const E *>(tabs)[sb[u * EPU + q]];
                __builtin_memcpy(out + g0 * ES + 16 * (int64_t)u, o, 16);
            }
            __syncthreads();
        } else {
            const int cnt = (int)(n - g0 < kTile ? n - g0 : kTile);
            for (int i = threadIdx.x; i < cnt; i += kBlock) {
                const unsigned b = in[g0 + i];
#pragma unroll
                for (int w = 0; w < WPE; w++) reinterpret_cast<S *>(out)[(g0 + i) * WPE + w] = reinterpret_cast<const S *>(tabs)[b * WPE + w];
            }
        }
    }
}

// ---------------------------------------------------------------- slicer
template <typename T> struct Promoted { typedef int type; };                  // int8, int16, int32: int
template <> struct Promoted<int64_t> { typedef long long type; };
template <> struct Promoted<float> { typedef float type; };
template <> struct Promoted<double> { typedef double type; };

// b - a in the promoted type; signed integers wrap
__device__ inline int diff(int b, int a) { return (int)((unsigned)b - (unsigned)a); }
__device__ inline long long diff(long long b, long long a) { return (long long)((unsigned long long)b - (unsigned long long)a); }
__device__ inline float diff(float b, float a)
{
#pragma clang fp contract(off)
    return b - a;
}
__device__ inline double diff(double b, double a)
{
#pragma clang fp contract(off)
    return b - a;
}
// (float)std::abs(d)
__device__ inline float abs_to_float(int d) { return (float)(d < 0 ? (int)(0u - (unsigned)d) : d); }
__device__ inline float abs_to_float(long long d) { return (float)(d < 0 ? (long long)(0ull - (unsigned long long)d) : d); }
__device__ inline float abs_to_float(float d) { return __builtin_fabsf(d); }
__device__ inline float abs_to_float(double d) { return (float)__builtin_fabs(d); }
// powf(dr, 2) + powf(di, 2) as the reference's compiler emits it: two products, one sum, each rounded on its own.  The pragma covers
// the front end; a build with -ffp-contract=fast also lets the back end fuse a product into the sum, so each product passes through
// an empty statement the optimiser cannot see through (no instruction is emitted for it).
__device__ inline float norm2(float dr, float di)
{
#pragma clang fp contract(off)
    float a = dr * dr;
    float b = di * di;
    __asm__("" : "+v"(a));
    __asm__("" : "+v"(b));
    return a + b;
}

template <typename T, bool CPLX>
struct SliceShape {
    static constexpr int W = CPLX ? 2 : 1, ES = (int)sizeof(T) * W;
    static constexpr int S = ES >= 4 ? 4 : 16 / ES;             // samples per lane
    static constexpr int LOADS = S * ES / 16;                   // 16-byte loads per lane
};

template <typename T, bool CPLX, bool ONCHIP>
__global__ __launch_bounds__(kBlock) void sym_slice_kernel(const T *__restrict__ in, unsigned char *__restrict__ out, int64_t n,
                                                            const typename Promoted<T>::type *__restrict__ mapc, int M)
{
    typedef typename Promoted<T>::type C;
    typedef SliceShape<T, CPLX> G;
    constexpr int W = G::W, S = G::S, LOADS = G::LOADS;
    __shared__ C lmap[ONCHIP ? kMaxOnChip * W : 1];
    if constexpr (ONCHIP) {
        for (int i = threadIdx.x; i < M * W; i += kBlock) lmap[i] = mapc[i];
        __syncthreads();
    }
    const C *mp = ONCHIP ? lmap : mapc;
    const int64_t ngroups = (n + S - 1) / S;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t i0 = g * S;
        const int cnt = n - i0 >= S ? S : (int)(n - i0);
        const bool whole = cnt == S;
        C xr[S], xi[S];
        if (whole) {
            T v[S * W];
            __builtin_memcpy(v, reinterpret_cast<const unsigned char *>(in) + i0 * (int64_t)(W * sizeof(T)), 16 * LOADS);
#pragma unroll
            for (int q = 0; q < S; q++) {
                xr[q] = (C)v[q * W];
                xi[q] = CPLX ? (C)v[q * W + W - 1] : (C)0;
            }
        } else {
#pragma unroll
            for (int q = 0; q < S; q++) {
                xr[q] = q < cnt ? (C)in[(i0 + q) * W] : (C)0;
                xi[q] = CPLX && q < cnt ? (C)in[(i0 + q) * W + W - 1] : (C)0;
            }
        }
        float best[S];
        uint32_t idx[S];
#pragma unroll
        for (int q = 0; q < S; q++) {
            best[q] = __FLT_MAX__;                // SymbolSlicer.cpp:89
            idx[q] = 0;
        }
        for (int j = 0; j < M; j++) {
            const C mr = mp[j * W];
            const C mi = CPLX ? mp[j * W + W - 1] : (C)0;
#pragma unroll
            for (int q = 0; q < S; q++) {
                float d;
                if constexpr (CPLX) d = norm2((float)diff(mr, xr[q]), (float)diff(mi, xi[q]));
                else d = abs_to_float(diff(mr, xr[q]));
                if (d < best[q]) {
                    best[q] = d;
                    idx[q] = (uint32_t)j;
                }
            }
        }
        if (whole) {
            uint32_t w[S / 4];
#pragma unroll
            for (int k = 0; k < S / 4; k++)
                w[k] = (idx[4 * k] & 255u) | ((idx[4 * k + 1] & 255u) << 8) | ((idx[4 * k + 2] & 255u) << 16) | ((idx[4 * k + 3] & 255u) << 24);
            __builtin_memcpy(out + i0, w, S);
        } else {
#pragma unroll
            for (int q = 0; q < S; q++)
                if (q < cnt) out[i0 + q] = (unsigned char)idx[q];
        }
    }
}

// ---------------------------------------------------------------- differential decoder
// halo[t] = the byte in front of tile t (the carried byte for tile 0); the carried byte := the slice's last
__global__ __launch_bounds__(kBlock) void diff_halo_kernel(const unsigned char *__restrict__ in, int64_t n, int64_t nt, uint32_t *state,
                                                            uint32_t *__restrict__ halo)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    if (t == 0) {
        halo[0] = state[0] & 255u;
        state[0] = in[n - 1];
    } else {
        halo[t] = in[t * kTile - 1];
    }
}
__global__ __launch_bounds__(kBlock) void diff_decode_kernel(const unsigned char *in, unsigned char *out, int64_t n, uint32_t symbols,
                                                              const uint32_t *__restrict__ halo)
{
    __shared__ uint32_t lastb[kBlock];
    const int64_t t = blockIdx.x, i0 = t * kTile + 16 * (int64_t)threadIdx.x;
    uint32_t w[4];
    const int cnt = load16(in, i0, n, w);
    lastb[threadIdx.x] = w[3] >> 24;
    __syncthreads();
    uint32_t prev = threadIdx.x ? lastb[threadIdx.x - 1] : halo[t];
    const bool pow2 = (symbols & (symbols - 1)) == 0;
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const uint32_t cur = (w[q >> 2] >> (8 * (q & 3))) & 255u;
        const uint32_t v = cur - prev + symbols;                      // modulo 2^32, as the reference's uint32_t
        const uint32_t r = pow2 ? v & (symbols - 1) : v % symbols;
        o[q >> 2] |= (r & 255u) << (8 * (q & 3));
        prev = cur;
    }
    store16(out, i0, cnt, o);
}

// ---------------------------------------------------------------- differential encoder
__device__ inline uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int k = kWave / 2; k >= 1; k >>= 1) v += (uint32_t)__shfl_xor((int)v, k, kWave);
    return v;
}
// SCAN, first pass: tsum[t] = the tile's byte sum mod m
__global__ __launch_bounds__(kBlock) void diff_tile_kernel(const unsigned char *__restrict__ in, int64_t n, uint32_t m, float rcp,
                                                            uint32_t *__restrict__ tsum)
{
    __shared__ uint32_t ws[kBlock / kWave];
    const int64_t t = blockIdx.x, i0 = t * kTile + 16 * (int64_t)threadIdx.x;
    uint32_t w[4];
    (void)load16(in, i0, n, w);
    const uint32_t s = wave_sum(byte_sum(w[0]) + byte_sum(w[1]) + byte_sum(w[2]) + byte_sum(w[3]));
    if ((threadIdx.x & (kWave - 1)) == 0) ws[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) tsum[t] = mod_small(ws[0] + ws[1] + ws[2] + ws[3], m, rcp);
}
// SCAN, second pass, one workgroup: tin[t] = (carry + the sums of the tiles in front of t) mod m; the carried byte := that behind the last
__global__ __launch_bounds__(kCarryThreads) void diff_carry_kernel(const uint32_t *__restrict__ tsum, int64_t nt, uint32_t m, float rcp, uint32_t *state,
                                                                    uint32_t *__restrict__ tin)
{
    __shared__ uint32_t sc[2][kCarryThreads];
    const int tid = threadIdx.x;
    const uint32_t carry = mod_small(state[0] & 255u, m, rcp);
    uint32_t v[kCarryRun], tot = 0;
#pragma unroll
    for (int k = 0; k < kCarryRun; k++) {
        const int64_t t = (int64_t)tid * kCarryRun + k;
        v[k] = t < nt ? tsum[t] : 0;
        tot += v[k];
    }
    tot = mod_small(tot, m, rcp);
    int cur = 0;
    sc[0][tid] = tot;
    __syncthreads();
    for (int d = 1; d < kCarryThreads; d <<= 1) {           // inclusive scan of the threads' totals: at most 1024 * 255
        sc[cur ^ 1][tid] = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t r = mod_small(carry + sc[cur][tid] - tot, m, rcp);
#pragma unroll
    for (int k = 0; k < kCarryRun; k++) {
        const int64_t t = (int64_t)tid * kCarryRun + k;
        if (t < nt) tin[t] = r;
        r = mod_small(r + v[k], m, rcp);
    }
    if (tid == kCarryThreads - 1) state[0] = r;             // (every thread read the carried byte before the first barrier)
}
// SCAN, third pass: the outputs of a tile
__global__ __launch_bounds__(kBlock) void diff_apply_kernel(const unsigned char *in, unsigned char *out, int64_t n, uint32_t m, float rcp,
                                                             const uint32_t *__restrict__ tin)
{
    __shared__ uint32_t ws[kBlock / kWave];
    const int64_t t = blockIdx.x, i0 = t * kTile + 16 * (int64_t)threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t w[4];
    const int cnt = load16(in, i0, n, w);
    const uint32_t mine = byte_sum(w[0]) + byte_sum(w[1]) + byte_sum(w[2]) + byte_sum(w[3]);
    uint32_t inc = mine;                                    // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d, kWave);
        if (lane >= d) inc += up;
    }
    if (lane == kWave - 1) ws[wave] = inc;
    __syncthreads();
    uint32_t front = tin[t] + inc - mine;                   // below 256 + 255 * 4096 < 2^21
    for (int k = 0; k < wave; k++) front += ws[k];
    uint32_t r = mod_small(front, m, rcp);
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; q++) {
        r = mod_small(r + ((w[q >> 2] >> (8 * (q & 3))) & 255u), m, rcp);
        o[q >> 2] |= r << (8 * (q & 3));
    }
    store16(out, i0, cnt, o);
}
// SERIAL: the reference's loop as written (DifferentialEncoder.cpp:59-63)
__global__ void diff_serial_kernel(const unsigned char *in, unsigned char *out, int64_t n, uint32_t symbols, uint32_t *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint8_t last = (uint8_t)state[0];
    for (int64_t i = 0; i < n; i++) {
        last = (uint8_t)(((uint32_t)in[i] + (uint32_t)last + symbols) % symbols);
        out[i] = last;
    }
    state[0] = last;
}

template <typename T>
int slice_launch(bool cplx, const void *in, void *out, size_t m, const void *mapc, size_t M, hipStream_t st)
{
    typedef typename Promoted<T>::type C;
    const T *x = static_cast<const T *>(in);
    unsigned char *y = static_cast<unsigned char *>(out);
    const C *mp = static_cast<const C *>(mapc);
    const bool onchip = M <= (size_t)kMaxOnChip;
    const int S = cplx ? SliceShape<T, true>::S : SliceShape<T, false>::S;
    const unsigned grid = stream_grid((m + S - 1) / S, kBlock);
    if (cplx) {
        if (onchip) hipLaunchKernelGGL((sym_slice_kernel<T, true, true>), dim3(grid), dim3(kBlock), 0, st, x, y, (int64_t)m, mp, (int)M);
        else hipLaunchKernelGGL((sym_slice_kernel<T, true, false>), dim3(grid), dim3(kBlock), 0, st, x, y, (int64_t)m, mp, (int)M);
    } else {
        if (onchip) hipLaunchKernelGGL((sym_slice_kernel<T, false, true>), dim3(grid), dim3(kBlock), 0, st, x, y, (int64_t)m, mp, (int)M);
        else hipLaunchKernelGGL((sym_slice_kernel<T, false, false>), dim3(grid), dim3(kBlock), 0, st, x, y, (int64_t)m, mp, (int)M);
    }
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

template <int SB>
int map_launch(bool cplx, const unsigned char *x, unsigned char *y, size_t m, const unsigned char *tab, hipStream_t st)
{
    const unsigned grid = stream_grid(((m + kTile - 1) / kTile) * kBlock, kBlock);
    if (cplx) hipLaunchKernelGGL((sym_map_kernel<SB, 2>), dim3(grid), dim3(kBlock), 0, st, x, y, (int64_t)m, tab);
    else hipLaunchKernelGGL((sym_map_kernel<SB, 1>), dim3(grid), dim3(kBlock), 0, st, x, y, (int64_t)m, tab);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace

size_t sym_tile() { return kTile; }
size_t sym_slice() { return (size_t)1 << kSliceLog; }
size_t slicer_max_onchip() { return kMaxOnChip; }
size_t slicer_lane_samples(int scalar, bool cplx)
{
    const int es = scalar_bytes(scalar) * (cplx ? 2 : 1);
    return es >= 4 ? 4 : 16 / es;
}
size_t slicer_block_samples(int scalar, bool cplx) { return slicer_lane_samples(scalar, cplx) * kBlock; }

int launch_sym_map(int scalar, bool cplx, const void *in, void *out, size_t m, const void *tab, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    const unsigned char *x = static_cast<const unsigned char *>(in), *tb = static_cast<const unsigned char *>(tab);
    unsigned char *y = static_cast<unsigned char *>(out);
    switch (scalar_bytes(scalar)) {
    case 8: return map_launch<8>(cplx, x, y, m, tb, st);
    case 4: return map_launch<4>(cplx, x, y, m, tb, st);
    case 2: return map_launch<2>(cplx, x, y, m, tb, st);
    case 1: return map_launch<1>(cplx, x, y, m, tb, st);
    }
    set_error("symbol mapper: unsupported type");
    return PCX_ERR_ARG;
}

int launch_sym_slice(int scalar, bool cplx, const void *in, void *out, size_t m, const void *mapc, size_t M, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    switch (scalar) {
    case PCX_F64: return slice_launch<double>(cplx, in, out, m, mapc, M, st);
    case PCX_F32: return slice_launch<float>(cplx, in, out, m, mapc, M, st);
    case PCX_I64: return slice_launch<int64_t>(cplx, in, out, m, mapc, M, st);
    case PCX_I32: return slice_launch<int32_t>(cplx, in, out, m, mapc, M, st);
    case PCX_I16: return slice_launch<int16_t>(cplx, in, out, m, mapc, M, st);
    case PCX_I8: return slice_launch<int8_t>(cplx, in, out, m, mapc, M, st);
    }
    set_error("symbol slicer: unsupported type");
    return PCX_ERR_ARG;
}

int launch_diff_slice(const DiffShape &p, const void *in, void *out, size_t m, uint32_t *state, uint32_t *tsum, uint32_t *tin, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    if (m > sym_slice()) {
        set_error("differential coder: a slice of %zu bytes", m);
        return PCX_ERR_ARG;
    }
    const unsigned char *x = static_cast<const unsigned char *>(in);
    unsigned char *y = static_cast<unsigned char *>(out);
    const int64_t nt = (int64_t)((m + kTile - 1) / kTile);
    if (p.decode) {
        hipLaunchKernelGGL(diff_halo_kernel, dim3((unsigned)((nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, x, (int64_t)m, nt, state, tin);
        PCX_LAUNCH_CHECK();
        hipLaunchKernelGGL(diff_decode_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, x, y, (int64_t)m, p.symbols, (const uint32_t *)tin);
        PCX_LAUNCH_CHECK();
        return PCX_OK;
    }
    if (p.plan == PCX_DIFF_SERIAL) {
        hipLaunchKernelGGL(diff_serial_kernel, dim3(1), dim3(64), 0, st, x, y, (int64_t)m, p.symbols, state);
        PCX_LAUNCH_CHECK();
        return PCX_OK;
    }
    const uint32_t mod = p.symbols < 256 ? p.symbols : 256;
    const float rcp = 1.0f / (float)mod;
    hipLaunchKernelGGL(diff_tile_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, x, (int64_t)m, mod, rcp, tsum);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL(diff_carry_kernel, dim3(1), dim3(kCarryThreads), 0, st, (const uint32_t *)tsum, nt, mod, rcp, state, tin);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL(diff_apply_kernel, dim3((unsigned)nt), dim3(kBlock), 0, st, x, y, (int64_t)m, mod, rcp, (const uint32_t *)tin);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace pcx
