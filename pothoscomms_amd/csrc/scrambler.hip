// scrambler.hip -- /comms/scrambler and /comms/descrambler (digital/Scrambler.cpp, Descrambler.cpp over digital/lfsr.h): a Galois LFSR
// stepped once per bit, one unsigned char per bit in and out, only bit 0 of an input byte counting.  Two plans:
//   SCAN    the polynomial owns the mask's lowest bit m and the seed lies below 2^m.  The register then stays below 2^m, ret is bit
//           m-1 of the old state and the step is linear over GF(2):  D' = M D ^ u e0,  out = b ^ ret, with u = 0 (additive) or u = b
//           (multiplicative; the descrambler's M has row 0 cleared, since its bit 0 is the input alone).  A thread owns a run of 256
//           bits packed into four words, a wave a tile of 64 runs; products with M^(2^k) are one row per lane, parity(row & v)
//           gathered by a ballot.  One call slice of at most 64 Mi bits runs as
//             additive        apply   the wave jumps the carried state to its tile (M^(tile offset) from the table of M^(2^k)), walks
//                                     it over the lanes with M^256, every lane steps its run and the bytes are stored
//                             finish  the carried state := the state behind the last bit
//             multiplicative  tile    every lane's run from zero state, then the walk over the lanes: the tile's zero-state end state
//                             carry   one workgroup of 16 waves: s_t = M^16384 s_(t-1) ^ z_t, 256 tiles per wave from zero state,
//                                     the waves joined with M^(256 * 16384), then the 256 tiles again from the wave's incoming state
//                             apply   the walk over the lanes from the tile's incoming state, the runs stepped, outputs stored
//                             finish  as above
//           Exact: every output bit and the carried state equal the reference's.
//   SERIAL  every other configuration: one thread runs the reference's loop as written, the full 64-bit mask included.
// No workgroup waits for another, the state lives at fixed addresses, every bit index is 64-bit.  out may be in itself (a tile is read
// whole before any of it is written) but must not overlap it otherwise.
#include "pcx_internal.hpp"

namespace pcx {
namespace {

constexpr int kRunLog = 8, kRun = 1 << kRunLog;                 // bits per lane
constexpr int kWave = 64;
constexpr int kTileLog = kRunLog + 6, kTile = 1 << kTileLog;    // bits per wave: 16384
constexpr int kTileWaves = 4;                                   // tiles per workgroup of the tile and apply kernels
constexpr int kGroupLog = 8, kGroup = 1 << kGroupLog;           // tiles per wave of the carry
constexpr int kCarryWaves = 16;
constexpr int kSliceLog = kTileLog + kGroupLog + 4;             // 2^26 bits = kCarryWaves * kGroup tiles
constexpr int kChunks = kTile / 16 / kWave;                     // 16-byte accesses per lane and tile: 16

static_assert(kCarryWaves == 16 && kSliceLog <= 26, "the power table of pcx_scr_api.hip holds M^(2^k) for k < 27");

typedef uint64_t __attribute__((may_alias)) u64a;
typedef uint16_t __attribute__((may_alias)) u16a;

// M v for a wave-uniform v: lane r holds row r
__device__ inline uint64_t wave_mv(uint64_t row, uint64_t v) { return __ballot((__popcll(row & v) & 1) != 0); }
__device__ inline uint64_t read_lane(uint64_t v, int i)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, i), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), i);
    return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t uniform(uint64_t v) { return read_lane(v, 0); }

// the walk over the lanes: s_0 = s0, s_(i+1) = M^256 s_i ^ z_i; lane i leaves with s_i in `mine`, all with s_64
__device__ inline uint64_t lane_walk(uint64_t z, uint64_t s0, uint64_t rowR, uint64_t &mine)
{
    const int lane = threadIdx.x & (kWave - 1);
    uint64_t s = s0;
    mine = 0;
#pragma unroll 4
    for (int i = 0; i < kWave; i++) {
        if (lane == i) mine = s;
        s = wave_mv(rowR, s) ^ read_lane(z, i);
    }
    return s;
}

// four bytes -> four bits (bit 0 of each), byte q to bit q; and back to bytes of 0 / 1
__device__ inline uint32_t pack4(uint32_t w) { return (((w & 0x01010101u) * 0x01020408u) >> 24) & 0xFu; }
__device__ inline uint32_t expand4(uint32_t nib) { return ((nib & 0xFu) * 0x00204081u) & 0x01010101u; }

// the tile [g0, g0 + 16384) of `in` as bits into the wave's LDS words (bit i of the tile = bit i % 64 of word i / 64); bytes at and
// past n read as 0
__device__ inline void load_tile(u64a *bits, const unsigned char *in, int64_t g0, int64_t n, bool aligned)
{
    const int lane = threadIdx.x & (kWave - 1);
    u16a *b16 = reinterpret_cast<u16a *>(bits);
    if (aligned && g0 + kTile <= n) {
        uint4 v[kChunks];
#pragma unroll
        for (int k = 0; k < kChunks; k++) v[k] = *reinterpret_cast<const uint4 *>(in + g0 + 16 * (int64_t)(k * kWave + lane));
#pragma unroll
        for (int k = 0; k < kChunks; k++)
            b16[k * kWave + lane] = (uint16_t)(pack4(v[k].x) | (pack4(v[k].y) << 4) | (pack4(v[k].z) << 8) | (pack4(v[k].w) << 12));
        return;
    }
#pragma unroll 1
    for (int k = 0; k < kChunks; k++) {
        const int64_t idx = g0 + 16 * (int64_t)(k * kWave + lane);
        uint32_t w = 0;
        for (int q = 0; q < 16; q++)
            if (idx + q < n) w |= (uint32_t)(in[idx + q] & 1u) << q;
        b16[k * kWave + lane] = (uint16_t)w;
    }
}
__device__ inline void store_tile(const u64a *bits, unsigned char *out, int64_t g0, int64_t n, bool aligned)
{
    const int lane = threadIdx.x & (kWave - 1);
    const u16a *b16 = reinterpret_cast<const u16a *>(bits);
    if (aligned && g0 + kTile <= n) {
#pragma unroll
        for (int k = 0; k < kChunks; k++) {
            const uint32_t w = b16[k * kWave + lane];
            *reinterpret_cast<uint4 *>(out + g0 + 16 * (int64_t)(k * kWave + lane)) =
                make_uint4(expand4(w), expand4(w >> 4), expand4(w >> 8), expand4(w >> 12));
        }
        return;
    }
#pragma unroll 1
    for (int k = 0; k < kChunks; k++) {
        const int64_t idx = g0 + 16 * (int64_t)(k * kWave + lane);
        const uint32_t w = b16[k * kWave + lane];
        for (int q = 0; q < 16; q++)
            if (idx + q < n) out[idx + q] = (unsigned char)((w >> q) & 1u);
    }
}

// what the step needs of a SCAN configuration
struct Lfsr {
    uint64_t pm;        // XORed in when bit m comes up: the polynomial (bit m and bit 0 included); the multiplicative descrambler's without bit 0
    uint32_t u;         // 1: the input bit is XORed into bit 0 (multiplicative); 0: additive
    int sh;             // m - 1: ret is this bit of the old state
    int narrow;         // m <= 31: the register fits 32 bits through the shift
};

// nb bits of word w (64 when FULL) through the register; the output bits come back in the same positions
template <typename T, bool FULL, bool OUT>
__device__ inline uint64_t step_word(T &D, uint64_t w, int nb, T pm, T u, int sh)
{
    uint64_t o = 0;
    if constexpr (FULL) {
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const T b = (T)((w >> j) & 1u), ret = (T)((D >> sh) & 1u);
            if constexpr (OUT) o |= (uint64_t)(b ^ ret) << j;
            D = (T)(D << 1) ^ (((T)0 - ret) & pm) ^ (b & u);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < nb; j++) {
            const T b = (T)((w >> j) & 1u), ret = (T)((D >> sh) & 1u);
            if constexpr (OUT) o |= (uint64_t)(b ^ ret) << j;
            D = (T)(D << 1) ^ (((T)0 - ret) & pm) ^ (b & u);
        }
    }
    return o;
}

// the lane's run: cnt (0 ... 256) bits of its four words from state D; with OUT the words are replaced by the output bits
template <typename T, bool OUT>
__device__ inline uint64_t step_run(uint64_t D0, u64a *words, int cnt, const Lfsr &k)
{
    T D = (T)D0;
    const T pm = (T)k.pm, u = (T)k.u;
#pragma unroll 1
    for (int w = 0; w < kRun / 64; w++) {
        const int nb = cnt - 64 * w;
        if (nb <= 0) break;
        const uint64_t x = words[w];
        const uint64_t o = nb >= 64 ? step_word<T, true, OUT>(D, x, 64, pm, u, k.sh) : step_word<T, false, OUT>(D, x, nb, pm, u, k.sh);
        if constexpr (OUT) words[w] = o;
    }
    return (uint64_t)D;
}
template <bool OUT>
__device__ inline uint64_t step_lane(uint64_t D0, u64a *words, int cnt, const Lfsr &k)
{
    return k.narrow ? step_run<uint32_t, OUT>(D0, words, cnt, k) : step_run<uint64_t, OUT>(D0, words, cnt, k);
}

__device__ inline int lane_count(int64_t g0, int64_t n)
{
    const int64_t left = n - (g0 + (int64_t)(threadIdx.x & (kWave - 1)) * kRun);
    return left <= 0 ? 0 : left >= kRun ? kRun : (int)left;
}

// multiplicative, first pass: zl[t][lane] = the lane's zero-state end state, z[t] = the tile's
__global__ __launch_bounds__(kTileWaves *kWave) void scr_tile_kernel(const unsigned char *in, int64_t n, int aligned, const uint64_t *__restrict__ pow,
                                                                      Lfsr k, uint64_t *__restrict__ z, uint64_t *__restrict__ zl)
{
    __shared__ u64a bits[kTileWaves][kTile / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    const int64_t t = (int64_t)blockIdx.x * kTileWaves + wave, g0 = t * kTile;
    const bool active = g0 < n;
    if (active) load_tile(bits[wave], in, g0, n, aligned != 0);
    __syncthreads();
    if (!active) return;
    const uint64_t e = step_lane<false>(0, &bits[wave][lane * (kRun / 64)], lane_count(g0, n), k);
    zl[t * kWave + lane] = e;
    uint64_t mine;
    const uint64_t end = lane_walk(e, 0, pow[kRunLog * kWave + lane], mine);
    if (lane == 0) z[t] = end;
}

// multiplicative, second pass: tin[t] = the state in front of tile t, from the carried state and the tiles' zero-state end states.  A
// wave holds its 256 z_t in four registers per lane (one coalesced load each) and walks them by readlane: no load on the chain.
__device__ inline uint64_t carry_walk(uint64_t s, const uint64_t (&zr)[kGroup / kWave], uint64_t (&tr)[kGroup / kWave], int count, uint64_t rowT)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int q = 0; q < kGroup / kWave; q++) {
        tr[q] = 0;
        const int left = count - q * kWave, lim = left < kWave ? left : kWave;
#pragma unroll 1
        for (int i = 0; i < lim; i++) {
            if (lane == i) tr[q] = s;
            s = wave_mv(rowT, s) ^ read_lane(zr[q], i);
        }
    }
    return s;
}
__global__ __launch_bounds__(kCarryWaves *kWave) void scr_carry_kernel(const uint64_t *__restrict__ z, int64_t nt, const uint64_t *__restrict__ state,
                                                                        const uint64_t *__restrict__ pow, uint64_t *__restrict__ tin)
{
    __shared__ uint64_t ends[kCarryWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    const int64_t t0 = (int64_t)wave * kGroup;
    const int count = nt - t0 >= kGroup ? kGroup : nt > t0 ? (int)(nt - t0) : 0;
    const uint64_t rowT = pow[kTileLog * kWave + lane], rowG = pow[(kTileLog + kGroupLog) * kWave + lane];
    uint64_t zr[kGroup / kWave], tr[kGroup / kWave];
#pragma unroll
    for (int q = 0; q < kGroup / kWave; q++) zr[q] = q * kWave + lane < count ? z[t0 + q * kWave + lane] : 0;
    uint64_t s = carry_walk(0, zr, tr, count, rowT);
    if (lane == 0) ends[wave] = s;
    __syncthreads();
    s = uniform(state[0]);
#pragma unroll 1
    for (int g = 0; g < wave; g++) s = wave_mv(rowG, s) ^ uniform(ends[g]);
    (void)carry_walk(s, zr, tr, count, rowT);
#pragma unroll
    for (int q = 0; q < kGroup / kWave; q++)
        if (q * kWave + lane < count) tin[t0 + q * kWave + lane] = tr[q];
}

// the outputs of a slice; next[0] = the state behind bit n - 1
__global__ __launch_bounds__(kTileWaves *kWave) void scr_apply_kernel(const unsigned char *in, unsigned char *out, int64_t n, int aligned,
                                                                       const uint64_t *__restrict__ pow, Lfsr k, const uint64_t *__restrict__ state,
                                                                       const uint64_t *__restrict__ tin, const uint64_t *__restrict__ zl,
                                                                       uint64_t *__restrict__ next)
{
    __shared__ u64a bits[kTileWaves][kTile / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    const int64_t t = (int64_t)blockIdx.x * kTileWaves + wave, g0 = t * kTile;
    const bool active = g0 < n;
    if (active) load_tile(bits[wave], in, g0, n, aligned != 0);
    __syncthreads();
    if (active) {
        uint64_t s0, e = 0;
        if (k.u == 0) {
            // additive: the keystream does not depend on the input; jump the carried state ahead by t tiles
            s0 = uniform(state[0]);
#pragma unroll 1
            for (int j = 0; j < kSliceLog - kTileLog; j++)
                if ((t >> j) & 1) s0 = wave_mv(pow[(kTileLog + j) * kWave + lane], s0);
        } else {
            s0 = uniform(tin[t]);
            e = zl[t * kWave + lane];
        }
        uint64_t mine;
        (void)lane_walk(e, s0, pow[kRunLog * kWave + lane], mine);
        const int cnt = lane_count(g0, n);
        const uint64_t D = step_lane<true>(mine, &bits[wave][lane * (kRun / 64)], cnt, k);
        if (cnt > 0 && g0 + (int64_t)lane * kRun + cnt == n) next[0] = D;
    }
    __syncthreads();
    if (active) store_tile(bits[wave], out, g0, n, aligned != 0);
}

__global__ void scr_finish_kernel(uint64_t *state)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) state[0] = state[1];
}

// SERIAL: GLFSR_next and the block loops as the reference writes them; kind 0 additive, 1 multiplicative scrambler, 2 descrambler
__global__ void scr_serial_kernel(const unsigned char *in, unsigned char *out, int64_t n, uint64_t *state, uint64_t polynomial, uint64_t mask,
                                  int kind)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t data = state[0];
    for (int64_t i = 0; i < n; i++) {
        const unsigned char b = in[i] & 0x1;
        unsigned char ret = 0;
        data <<= 1;
        if (data & mask) {
            ret = 1;
            data ^= polynomial;
        }
        const unsigned char o = b ^ ret;
        if (kind == 1) data = (data & ~uint64_t(1)) | o;
        else if (kind == 2) data = (data & ~uint64_t(1)) | b;
        out[i] = o;
    }
    state[0] = data;
}

}  // namespace

size_t scr_run() { return kRun; }
size_t scr_tile() { return kTile; }
size_t scr_group() { return (size_t)kGroup * kTile; }
size_t scr_slice() { return (size_t)1 << kSliceLog; }

int launch_scr_slice(const ScrShape &p, const void *in, void *out, size_t m, uint64_t *state, const uint64_t *pow, uint64_t *z, uint64_t *tin,
                     uint64_t *zl, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    if (m > scr_slice()) {
        set_error("scrambler: a slice of %zu bits", m);
        return PCX_ERR_ARG;
    }
    const unsigned char *x = static_cast<const unsigned char *>(in);
    unsigned char *y = static_cast<unsigned char *>(out);
    const bool mult = p.mode == PCX_SCR_MULTIPLICATIVE;
    if (p.plan == PCX_SCR_SERIAL) {
        hipLaunchKernelGGL(scr_serial_kernel, dim3(1), dim3(64), 0, st, x, y, (int64_t)m, state, p.polynomial, p.mask,
                           mult ? (p.descramble ? 2 : 1) : 0);
        PCX_LAUNCH_CHECK();
        return PCX_OK;
    }
    Lfsr k;
    k.pm = mult && p.descramble ? p.polynomial & ~uint64_t(1) : p.polynomial;
    k.u = mult ? 1u : 0u;
    k.sh = p.m - 1;
    k.narrow = p.m <= 31;
    const int aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int64_t nt = (int64_t)((m + kTile - 1) / kTile);
    const unsigned grid = (unsigned)((nt + kTileWaves - 1) / kTileWaves);
    if (mult) {
        hipLaunchKernelGGL(scr_tile_kernel, dim3(grid), dim3(kTileWaves * kWave), 0, st, x, (int64_t)m, aligned, pow, k, z, zl);
        PCX_LAUNCH_CHECK();
        hipLaunchKernelGGL(scr_carry_kernel, dim3(1), dim3(kCarryWaves * kWave), 0, st, (const uint64_t *)z, nt, (const uint64_t *)state, pow, tin);
        PCX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scr_apply_kernel, dim3(grid), dim3(kTileWaves * kWave), 0, st, x, y, (int64_t)m, aligned, pow, k, (const uint64_t *)state,
                       (const uint64_t *)tin, (const uint64_t *)zl, state + 1);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL(scr_finish_kernel, dim3(1), dim3(64), 0, st, state);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace pcx
