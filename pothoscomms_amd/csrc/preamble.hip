// preamble.hip -- /comms/preamble_correlator (digital/PreambleCorrelator.cpp): for every input position n the Hamming distance
//   dist[n] = sum over i < P of popcount(preamble[i] ^ in[n + i])        (whole bytes: the upper bits of an input byte count)
// and, in ascending order, the positions with dist <= threshold.  One call slice of at most 64 Mi positions runs as
//   distance  a workgroup owns a tile of 4096 positions.  It stages the tile's bytes and the P - 1 behind them once into LDS (and
//             copies the tile to `out` when asked), then works per BIT PLANE of the symbols:
//               a plane in which the preamble has a set bit ("active") is packed 32 positions to a word by one ballot per 64 bytes; a lane
//               owns the bit offset s = lane % 32 and 16 positions 32 apart, so one v_alignbit per word gives the 32-bit window that
//               serves a position with preamble word k and the next position with word k - 1: xor + bcnt per 32 preamble symbols;
//               the planes in which the preamble is all zero contribute the number of ones in the window, together: a prefix sum of
//               popcount(byte & inactive planes) over the staged bytes, kept mod 2^16, and one difference per position.
//             The matches of a tile leave as 128 words of one bit per position and a count (or, for pcx_preamble_distances, the
//             distances themselves leave as uint32).
//   offsets   one workgroup: the exclusive scan of the tile counts, the running total of the call carried in device memory
//   select    a tile with matches ranks its set bits behind its offset and stores n + P as uint64 while the rank is below idx_cap
// so the order of the indices does not depend on the order in which workgroups ran.  A preamble longer than 1024 symbols takes the
// BYTES plan: the distance step is the reference's loop, one position per thread, the other two steps are shared.
// Exact for every byte value and every P >= 1; no workgroup waits for another; every stream index is 64-bit.
#include "pcx_internal.hpp"

namespace pcx {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;                         // four waves
constexpr int kR = 16;                                // positions per lane, 32 apart
constexpr int kTile = kThreads * kR;                  // 4096 positions per workgroup
constexpr int kMaskWords = kTile / 32;                // 128
constexpr int kMaxP = 1024;                           // PLANES plan: the halo that fits the tile's LDS
constexpr int kKMax = kMaxP / 32;                     // preamble words per plane
constexpr int kStage = kTile + kMaxP;                 // staged bytes (the last one is never needed: P - 1 behind the tile)
constexpr int kPlaneWords = kStage / 32;              // 160
constexpr int kSliceLog = 26;
constexpr int kScanThreads = 1024;
constexpr int kScanPer = (1 << kSliceLog) / kTile / kScanThreads;      // tile counts per thread of the offsets step: 16

static_assert(kScanPer * kScanThreads * kTile == 1 << kSliceLog, "the offsets step covers a slice with one workgroup");
static_assert(kStage % 16 == 0 && kStage == 20 * kThreads, "16-byte staging chunks; the prefix step gives a thread 20 bytes");

typedef uint32_t __attribute__((may_alias)) u32a;
typedef uint16_t __attribute__((may_alias)) u16a;
typedef uint64_t __attribute__((may_alias)) u64a;

// what the distance step needs of a configured preamble
struct PreK {
    int P;                    // symbols
    int kfull;                // whole 32-symbol words: P / 32
    uint32_t tail;            // mask of the symbols behind them: (1 << P % 32) - 1
    uint32_t active;          // bit b: the preamble has a set bit in plane b
    uint32_t thr;
};

// the tile's matches (one bit per position in `lm`) and their number leave the workgroup
__device__ inline void store_matches(const uint32_t *lm, int *lcount, int64_t tile, uint32_t *__restrict__ mask, uint32_t *__restrict__ counts)
{
    __syncthreads();
    if (threadIdx.x < kMaskWords) {
        const uint32_t w = lm[threadIdx.x];
        mask[tile * kMaskWords + threadIdx.x] = w;
        if (w) atomicAdd(lcount, __popc(w));
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[tile] = (uint32_t)*lcount;
}

// KC preamble words from word k on for the lane's kR positions: kR + KC words of the plane, one window per word
template <int KC, bool MASKED>
__device__ inline void plane_chunk(uint32_t (&d)[kR], const u32a *xw, const uint32_t *__restrict__ pw, int k, uint32_t s, uint32_t tail)
{
    uint32_t w[kR + KC];
#pragma unroll
    for (int i = 0; i < kR + KC; i++) w[i] = xw[k + i];
#pragma unroll
    for (int i = 0; i < kR + KC - 1; i++) w[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], s);
#pragma unroll
    for (int kk = 0; kk < KC; kk++) {
        const uint32_t p = pw[k + kk];          // the same word in every lane
#pragma unroll
        for (int r = 0; r < kR; r++) d[r] += MASKED ? __popc((w[r + kk] ^ p) & tail) : __popc(w[r + kk] ^ p);
    }
}

// PLANES: m positions of the slice from in[0]; in[0 .. m + P) exists.  DIST: the distances leave instead of the matches.
template <bool DIST>
__global__ __launch_bounds__(kThreads) void pre_planes_kernel(const unsigned char *in, unsigned char *out, int64_t m, int aligned, PreK c,
                                                              const uint32_t *__restrict__ pw, uint32_t *__restrict__ mask,
                                                              uint32_t *__restrict__ counts, uint32_t *__restrict__ dist)
{
    __shared__ __attribute__((aligned(16))) unsigned char raw[kStage];
    __shared__ u64a planes[8][kPlaneWords / 2];
    __shared__ u16a pref[kStage + 2];
    __shared__ uint32_t lm[kMaskWords];
    __shared__ int wsum[kThreads / kWave];
    __shared__ int lcount;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    const int64_t tile = blockIdx.x, g0 = tile * kTile, avail = m + c.P;       // bytes of `in` that exist
    const int need = kTile + c.P - 1;                                          // staged bytes a full tile reads
    if (tid == 0) lcount = 0;

    // stage (zero behind the data), and forward the tile
#pragma unroll 1
    for (int q = tid; q * 16 < need; q += kThreads) {
        const int64_t g = g0 + 16 * (int64_t)q;
        uint32_t e[4] = {0, 0, 0, 0};
        if (aligned && g + 16 <= avail) {
            const uint4 v = *reinterpret_cast<const uint4 *>(in + g);
            e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (g + i < avail) e[i >> 2] |= (uint32_t)in[g + i] << (8 * (i & 3));
        }
        *reinterpret_cast<uint4 *>(raw + 16 * q) = make_uint4(e[0], e[1], e[2], e[3]);
        if (out && 16 * q < kTile) {
            if (aligned && g + 16 <= m) {
                *reinterpret_cast<uint4 *>(out + g) = make_uint4(e[0], e[1], e[2], e[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (g + i < m) out[g + i] = (unsigned char)(e[i >> 2] >> (8 * (i & 3)));
            }
        }
    }
    __syncthreads();

    // the active planes, 64 positions per ballot
    const int groups = (need + kWave - 1) / kWave;
#pragma unroll 1
    for (int g = wave; g < groups; g += kThreads / kWave) {
        const uint32_t x = raw[g * kWave + lane];
#pragma unroll
        for (int b = 0; b < 8; b++) {
            if (!((c.active >> b) & 1)) continue;
            const uint64_t w = __ballot(((x >> b) & 1u) != 0);
            if (lane == 0) planes[b][g] = w;
        }
    }
    // the inactive planes: pref[j] = ones in them over raw[0 .. j), mod 2^16 (a window holds at most 8 * 1024)
    const uint32_t idle = ~c.active & 0xFFu;
    if (idle) {
        constexpr int kPer = kStage / kThreads;           // 20 bytes per thread
        const uint32_t idle4 = idle * 0x01010101u;
        const u32a *rw = reinterpret_cast<const u32a *>(raw) + tid * (kPer / 4);
        uint32_t v[kPer / 4];
        int sum = 0;
#pragma unroll
        for (int i = 0; i < kPer / 4; i++) {
            v[i] = rw[i] & idle4;
            sum += __popc(v[i]);
        }
        int inc = sum;                                    // inclusive scan over the wave, then over the four waves
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int t = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += t;
        }
        if (lane == kWave - 1) wsum[wave] = inc;
        __syncthreads();
        int base = inc - sum;
        for (int i = 0; i < wave; i++) base += wsum[i];
        u16a *pp = pref + tid * kPer;
#pragma unroll
        for (int i = 0; i < kPer / 4; i++) {
            pp[4 * i + 0] = (uint16_t)base;
            pp[4 * i + 1] = (uint16_t)(base + __popc(v[i] & 0xFFu));
            pp[4 * i + 2] = (uint16_t)(base + __popc(v[i] & 0xFFFFu));
            pp[4 * i + 3] = (uint16_t)(base + __popc(v[i] & 0xFFFFFFu));
            base += __popc(v[i]);
        }
        if (tid == kThreads - 1) pref[kStage] = (uint16_t)base;
    }
    __syncthreads();

    // the distances of the lane's kR positions: (wb + r) * 32 + s
    const uint32_t s = lane & 31, h = lane >> 5;
    const int wb = (wave * 2 + (int)h) * kR;
    uint32_t d[kR];
#pragma unroll
    for (int r = 0; r < kR; r++) d[r] = 0;
#pragma unroll 1
    for (int b = 0; b < 8; b++) {
        if (!((c.active >> b) & 1)) continue;
        const u32a *xw = reinterpret_cast<const u32a *>(planes[b]) + wb;
        const uint32_t *pb = pw + b * kKMax;
        int k = 0;
#pragma unroll 1
        for (; k + 4 <= c.kfull; k += 4) plane_chunk<4, false>(d, xw, pb, k, s, 0);
        if (k + 2 <= c.kfull) { plane_chunk<2, false>(d, xw, pb, k, s, 0); k += 2; }
        if (k < c.kfull) { plane_chunk<1, false>(d, xw, pb, k, s, 0); k += 1; }
        if (c.tail) plane_chunk<1, true>(d, xw, pb, k, s, c.tail);
    }
    if (idle) {
#pragma unroll
        for (int r = 0; r < kR; r++) {
            const int nl = (wb + r) * 32 + (int)s;
            d[r] += (uint16_t)(pref[nl + c.P] - pref[nl]);
        }
    }
#pragma unroll
    for (int r = 0; r < kR; r++) {
        const int64_t g = g0 + (wb + r) * 32 + (int)s;
        const bool valid = g < m;
        if constexpr (DIST) {
            if (valid) dist[g] = d[r];
        } else {
            const uint64_t hit = __ballot(valid && d[r] <= c.thr);
            if (s == 0) lm[wb + r] = (uint32_t)(hit >> (32 * h));
        }
    }
    if constexpr (!DIST) store_matches(lm, &lcount, tile, mask, counts);
}

// BYTES: the reference's loop, one position per thread and row; pre: the P preamble bytes
template <bool DIST>
__global__ __launch_bounds__(kThreads) void pre_bytes_kernel(const unsigned char *in, unsigned char *out, int64_t m, PreK c,
                                                             const unsigned char *__restrict__ pre, uint32_t *__restrict__ mask,
                                                             uint32_t *__restrict__ counts, uint32_t *__restrict__ dist)
{
    __shared__ uint32_t lm[kMaskWords];
    __shared__ int lcount;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int64_t tile = blockIdx.x, g0 = tile * kTile;
    if (tid == 0) lcount = 0;
#pragma unroll 1
    for (int r = 0; r < kR; r++) {
        const int nl = r * kThreads + tid;
        const int64_t g = g0 + nl;
        const bool valid = g < m;
        uint32_t d = 0;
        if (valid) {
            for (int i = 0; i < c.P; i++) d += __popc((uint32_t)(pre[i] ^ in[g + i]));
            if (out) out[g] = in[g];
        }
        if constexpr (DIST) {
            if (valid) dist[g] = d;
        } else {
            const uint64_t hit = __ballot(valid && d <= c.thr);
            if ((lane & 31) == 0) lm[nl >> 5] = (uint32_t)(hit >> (lane & 32));
        }
    }
    if constexpr (!DIST) store_matches(lm, &lcount, tile, mask, counts);
}

// offsets: toff[t] = matches of the slice in front of tile t; state[0] = matches of the call so far, state[1] = those in front of
// this slice.  The last slice of a call hands out the call's two counts.
__global__ __launch_bounds__(kScanThreads) void pre_offsets_kernel(const uint32_t *__restrict__ counts, int64_t nt, int first, uint64_t *state,
                                                                    uint32_t *__restrict__ toff, uint64_t npos, uint64_t *npos_out, uint64_t *nmatch_out)
{
    __shared__ uint32_t part[kScanThreads];
    const int tid = threadIdx.x;
    uint32_t v[kScanPer], sum = 0;
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        const int64_t t = (int64_t)tid * kScanPer + i;
        v[i] = t < nt ? counts[t] : 0;
        sum += v[i];
    }
    part[tid] = sum;
    __syncthreads();
#pragma unroll 1
    for (int o = 1; o < kScanThreads; o <<= 1) {
        const uint32_t t = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        const int64_t t = (int64_t)tid * kScanPer + i;
        if (t < nt) toff[t] = run;
        run += v[i];
    }
    if (tid == kScanThreads - 1) {
        const uint64_t before = first ? 0 : state[0], total = before + part[tid];
        state[1] = before;
        state[0] = total;
        if (npos_out) *npos_out = npos;
        if (nmatch_out) *nmatch_out = total;
    }
}

// select: label indices pos0 + n + P of one tile, ranked behind state[1] + toff[tile]
__global__ __launch_bounds__(kMaskWords) void pre_select_kernel(const uint32_t *__restrict__ mask, const uint32_t *__restrict__ counts,
                                                                const uint32_t *__restrict__ toff, const uint64_t *__restrict__ state, uint64_t pos0,
                                                                uint64_t P, uint64_t *__restrict__ idx, uint64_t cap)
{
    __shared__ uint32_t cnt[kMaskWords];
    const int64_t tile = blockIdx.x;
    if (counts[tile] == 0) return;
    const int tid = threadIdx.x;
    uint32_t w = mask[tile * kMaskWords + tid];
    cnt[tid] = (uint32_t)__popc(w);
    __syncthreads();
    uint64_t rank = state[1] + toff[tile];
    for (int i = 0; i < tid; i++) rank += cnt[i];
    const uint64_t at = pos0 + (uint64_t)tile * kTile + 32u * (uint64_t)tid + P;
    while (w && rank < cap) {
        const int bit = __ffs((int)w) - 1;
        idx[rank++] = at + (uint64_t)bit;
        w &= w - 1;
    }
}

// a call without a position
__global__ void pre_empty_kernel(uint64_t *state, uint64_t *npos_out, uint64_t *nmatch_out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    state[0] = state[1] = 0;
    if (npos_out) *npos_out = 0;
    if (nmatch_out) *nmatch_out = 0;
}

PreK kernel_shape(const PreShape &p)
{
    PreK c;
    c.P = (int)p.P;
    c.kfull = (int)(p.P / 32);
    c.tail = p.P % 32 ? (1u << (p.P % 32)) - 1u : 0u;
    c.active = p.active;
    c.thr = p.threshold;
    return c;
}

}  // namespace

size_t pre_tile() { return kTile; }
size_t pre_slice() { return (size_t)1 << kSliceLog; }
size_t pre_max_planes_len() { return kMaxP; }
size_t pre_table_words() { return 8 * kKMax; }

int launch_pre_empty(uint64_t *state, uint64_t *npos_out, uint64_t *nmatch_out, hipStream_t st)
{
    hipLaunchKernelGGL(pre_empty_kernel, dim3(1), dim3(64), 0, st, state, npos_out, nmatch_out);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

int launch_pre_slice(const PreShape &p, const void *in, void *out, size_t m, const uint32_t *pw, const unsigned char *pre, const PreWork &w, uint64_t pos0,
                     int first, uint64_t npos, uint64_t *npos_out, uint64_t *nmatch_out, uint64_t *idx, uint64_t cap, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    if (m > pre_slice()) {
        set_error("preamble correlator: a slice of %zu positions", m);
        return PCX_ERR_ARG;
    }
    const unsigned char *x = static_cast<const unsigned char *>(in);
    unsigned char *y = static_cast<unsigned char *>(out);
    const PreK c = kernel_shape(p);
    const int64_t nt = (int64_t)((m + kTile - 1) / kTile);
    if (p.plan == PCX_PRE_PLANES) {
        const int aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
        hipLaunchKernelGGL(pre_planes_kernel<false>, dim3((unsigned)nt), dim3(kThreads), 0, st, x, y, (int64_t)m, aligned, c, pw, w.mask, w.counts,
                           (uint32_t *)nullptr);
    } else {
        hipLaunchKernelGGL(pre_bytes_kernel<false>, dim3((unsigned)nt), dim3(kThreads), 0, st, x, y, (int64_t)m, c, pre, w.mask, w.counts,
                           (uint32_t *)nullptr);
    }
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL(pre_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t *)w.counts, nt, first, w.state, w.toff, npos, npos_out,
                       nmatch_out);
    PCX_LAUNCH_CHECK();
    if (cap) {
        hipLaunchKernelGGL(pre_select_kernel, dim3((unsigned)nt), dim3(kMaskWords), 0, st, (const uint32_t *)w.mask, (const uint32_t *)w.counts,
                           (const uint32_t *)w.toff, (const uint64_t *)w.state, pos0, (uint64_t)p.P, idx, cap);
        PCX_LAUNCH_CHECK();
    }
    return PCX_OK;
}

int launch_pre_distances(const PreShape &p, const void *in, size_t m, const uint32_t *pw, const unsigned char *pre, uint32_t *dist, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    if (m > pre_slice()) {
        set_error("preamble correlator: a slice of %zu positions", m);
        return PCX_ERR_ARG;
    }
    const unsigned char *x = static_cast<const unsigned char *>(in);
    const PreK c = kernel_shape(p);
    const unsigned nt = (unsigned)((m + kTile - 1) / kTile);
    if (p.plan == PCX_PRE_PLANES) {
        const int aligned = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
        hipLaunchKernelGGL(pre_planes_kernel<true>, dim3(nt), dim3(kThreads), 0, st, x, (unsigned char *)nullptr, (int64_t)m, aligned, c, pw,
                           (uint32_t *)nullptr, (uint32_t *)nullptr, dist);
    } else {
        hipLaunchKernelGGL(pre_bytes_kernel<true>, dim3(nt), dim3(kThreads), 0, st, x, (unsigned char *)nullptr, (int64_t)m, c, pre, (uint32_t *)nullptr,
                           (uint32_t *)nullptr, dist);
    }
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace pcx
