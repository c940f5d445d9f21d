// threshold.hip -- /comms/threshold (utility/Threshold.cpp:111-149): a real stream is compared against an activation and a
// deactivation level, one bit of state is carried, and the elements at which the state changes are listed in ascending order
// (DESIGN.md 17).  With a = (x > activation) and d = (x < deactivation) an element is a MAP on {inactive, active}:
//   inactive -> a        active -> !d        (keep: a = d = 0, set: a = 1, d = 0, clear: a = 0, d = 1, toggle: a = d = 1)
// and the state after an element is the composition of the maps in front of it applied to the state on entry.  64 maps lie in two
// words (f0: the images of inactive, f1: those of active) and are composed by a six-step prefix inside the word.  One call slice of
// at most 64 Mi elements runs as
//   classify  a workgroup owns a tile of 4096 elements: 16-byte units at any address, forwarded to `out` when asked; a lane's
//             comparisons of a unit meet in LDS as the tile's two mask rows (64 words each), which one wave composes: per word,
//             then over the 64 words.  The rows, the tile's map and its number of transitions FOR EITHER ENTRY STATE leave.
//   offsets   one workgroup folds the tile maps from the carried state, which gives every tile its entry state and with it its
//             count; the exclusive scan of the counts, the call's running total and the state behind the slice stay on the device
//   select    a tile with transitions replays its rows from its entry state and ranks the set bits behind its offset: stream
//             indices as uint64 while the rank is below idx_cap
// so the order of the indices does not depend on the order in which workgroups ran.  pcx_threshold_states runs classify and offsets
// and then writes the state after every element, one byte each.  Exact for the six element types (the comparisons are the
// element type's own: a NaN compares false, int64 stays int64); no workgroup waits for another; every stream index is 64-bit.
#include "pcx_internal.hpp"
#include "unit_io.hpp"

namespace pcx {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;                         // four waves
constexpr int kTile = 4096;                           // elements per workgroup
constexpr int kWords = kTile / 64;                    // words per mask row: one per lane of a wave
constexpr int kSliceLog = 26;
constexpr int kScanThreads = 1024;
constexpr int kScanPer = (1 << kSliceLog) / kTile / kScanThreads;      // tiles per thread of the offsets step: 16

static_assert(kWords == kWave, "one wave composes a tile, a word per lane");
static_assert(kScanPer * kScanThreads * kTile == 1 << kSliceLog, "the offsets step covers a slice with one workgroup");

// a tile's record: transitions when entered inactive | when entered active << 13 | image of inactive << 26 | image of active << 27
constexpr int kCnt1Shift = 13, kMap0Bit = 26, kMap1Bit = 27;
constexpr uint32_t kCntMask = 0x1FFFu, kIdentityRec = 1u << kMap1Bit;
// a tile's offset: transitions of the slice in front of it | its entry state << 31
constexpr uint32_t kOffMask = 0x7FFFFFFFu;

static_assert(kTile <= (int)kCntMask, "a tile's count fits its field");

typedef uint16_t __attribute__((may_alias)) u16a;
typedef uint64_t __attribute__((aligned(1), may_alias)) u64any;

// the 64 maps (f0, f1) of a word composed up to and including every element: bit i of p0 / p1 = the state after element i of a
// word entered inactive / active.  A step composes every prefix with the one 2^k elements in front (the identity where none is).
__device__ inline void word_prefix(uint64_t f0, uint64_t f1, uint64_t &p0, uint64_t &p1)
{
    p0 = f0;
    p1 = f1;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint64_t q0 = p0 << s, q1 = (p1 << s) | ((1ull << s) - 1);
        const uint64_t h0 = (q0 & p1) | (~q0 & p0), h1 = (q1 & p1) | (~q1 & p0);
        p0 = h0;
        p1 = h1;
    }
}

// A whole wave, lane l holding the prefixes of word l of a tile: bit l of x0 / x1 = the state in which word l is entered by a tile
// entered inactive / active; t0 / t1: the tile's own map
__device__ inline void tile_prefix(uint64_t p0, uint64_t p1, uint64_t &x0, uint64_t &x1, uint32_t &t0, uint32_t &t1)
{
    const uint64_t w0 = __ballot((p0 >> 63) != 0), w1 = __ballot((p1 >> 63) != 0);
    uint64_t P0, P1;
    word_prefix(w0, w1, P0, P1);
    x0 = P0 << 1;
    x1 = (P1 << 1) | 1ull;
    t0 = (uint32_t)(P0 >> 63);
    t1 = (uint32_t)(P1 >> 63);
}

// the states after the elements of a word entered in state s, and the elements at which the state changed
__device__ inline uint64_t word_states(uint64_t p0, uint64_t p1, uint32_t s) { return s ? p1 : p0; }
__device__ inline uint64_t word_changes(uint64_t S, uint32_t s) { return S ^ ((S << 1) | (uint64_t)s); }

// lane l of a wave: word l of the tile's rows replayed from the tile's entry state e
__device__ inline void replay(const uint64_t *__restrict__ mask, int64_t tile, int lane, uint32_t e, uint64_t &S, uint64_t &T)
{
    const uint64_t A = mask[tile * (2 * kWords) + lane], D = mask[tile * (2 * kWords) + kWords + lane];
    uint64_t p0, p1, x0, x1;
    uint32_t t0, t1;
    word_prefix(A, ~D, p0, p1);
    tile_prefix(p0, p1, x0, x1, t0, t1);
    const uint32_t s = (uint32_t)(((e ? x1 : x0) >> lane) & 1u);
    S = word_states(p0, p1, s);
    T = word_changes(S, s);
}

// classify: m elements of the slice from in[0]
template <typename T>
__global__ __launch_bounds__(kThreads) void thr_classify_kernel(const unsigned char *in, unsigned char *out, int64_t m, T act, T deact,
                                                                uint64_t *__restrict__ mask, uint32_t *__restrict__ rec)
{
    constexpr int E = 16 / (int)sizeof(T);            // elements per 16-byte unit
    constexpr int R = (int)sizeof(T);                 // units per lane: kTile * sizeof(T) / 16 / kThreads
    __shared__ uint64_t la[kWords], ld[kWords];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int64_t tile = blockIdx.x, e0 = tile * kTile, nbytes = m * (int64_t)sizeof(T), b0 = e0 * (int64_t)sizeof(T);

    uint4 v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = load_unit(in, b0 + 16 * (int64_t)(r * kThreads + tid), nbytes);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int u = r * kThreads + tid;
        if (out) store_unit(out, b0 + 16 * (int64_t)u, nbytes, v[r]);
        T x[E];
        __builtin_memcpy(x, &v[r], 16);
        const int64_t left = m - (e0 + (int64_t)u * E);                 // elements of the unit that exist: the rest keep the state
        const uint32_t valid = left >= E ? (1u << E) - 1u : left <= 0 ? 0u : (1u << left) - 1u;
        uint32_t a = 0, d = 0;
#pragma unroll
        for (int j = 0; j < E; j++) {
            a |= (uint32_t)(x[j] > act) << j;
            d |= (uint32_t)(x[j] < deact) << j;
        }
        a &= valid;
        d &= valid;
        // the unit's E flags lie at bit u * E of the row
        if constexpr (E == 16) {
            reinterpret_cast<u16a *>(la)[u] = (uint16_t)a;
            reinterpret_cast<u16a *>(ld)[u] = (uint16_t)d;
        } else {
#pragma unroll
            for (int w = E; w < 8; w *= 2) {          // neighbouring lanes' flags join to a byte
                a |= __shfl_down(a, w / E, kWave) << w;
                d |= __shfl_down(d, w / E, kWave) << w;
            }
            constexpr int kPerByte = E < 8 ? 8 / E : 1;
            if (lane % kPerByte == 0) {
                reinterpret_cast<unsigned char *>(la)[u / kPerByte] = (unsigned char)a;
                reinterpret_cast<unsigned char *>(ld)[u / kPerByte] = (unsigned char)d;
            }
        }
    }
    __syncthreads();
    if (tid >= kWave) return;

    const uint64_t A = la[lane], D = ld[lane];
    mask[tile * (2 * kWords) + lane] = A;
    mask[tile * (2 * kWords) + kWords + lane] = D;
    uint64_t p0, p1, x0, x1;
    uint32_t t0, t1;
    word_prefix(A, ~D, p0, p1);
    tile_prefix(p0, p1, x0, x1, t0, t1);
    const uint32_t s0 = (uint32_t)((x0 >> lane) & 1u), s1 = (uint32_t)((x1 >> lane) & 1u);
    uint32_t c = (uint32_t)__popcll(word_changes(word_states(p0, p1, s0), s0)) |
                 (uint32_t)__popcll(word_changes(word_states(p0, p1, s1), s1)) << 16;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    if (lane == 0) rec[tile] = (c & 0xFFFFu) | (c >> 16) << kCnt1Shift | t0 << kMap0Bit | t1 << kMap1Bit;
}

// offsets: toff[t] = transitions of the slice in front of tile t | the state in which tile t is entered << 31.  *src: the state in
// which the slice is entered, *dst: receives the state behind it.  tot (process only): [0] transitions of the call so far, [1] those
// in front of this slice, [2] the state in which the call was entered; the last slice of a call hands out the call's three counts.
// Two barriers: the maps of the waves in front give a thread its entry state, the sums of the waves in front its offset.
__global__ __launch_bounds__(kScanThreads) void thr_offsets_kernel(const uint32_t *__restrict__ rec, int64_t nt, int first, const uint64_t *src,
                                                                    uint64_t *dst, uint64_t *tot, uint32_t *__restrict__ toff, uint64_t nelem,
                                                                    uint64_t *counts_out)
{
    constexpr int kWaves = kScanThreads / kWave;
    __shared__ uint32_t wmap[kWaves], wsum[kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
    const uint32_t entry = (uint32_t)(*src & 1u);
    uint32_t r[kScanPer], g0 = 0, g1 = 1;              // the thread's tiles composed
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        const int64_t t = (int64_t)tid * kScanPer + i;
        r[i] = t < nt ? rec[t] : kIdentityRec;
        const uint32_t f0 = (r[i] >> kMap0Bit) & 1u, f1 = (r[i] >> kMap1Bit) & 1u;
        g0 = g0 ? f1 : f0;
        g1 = g1 ? f1 : f0;
    }
    uint64_t P0, P1;
    word_prefix(__ballot(g0 != 0), __ballot(g1 != 0), P0, P1);
    if (lane == 0) wmap[wave] = (uint32_t)(P0 >> 63) | (uint32_t)(P1 >> 63) << 1;
    __syncthreads();
    uint32_t s = entry;
    for (int w = 0; w < wave; w++) s = (wmap[w] >> s) & 1u;
    s = (uint32_t)((((s ? (P1 << 1) | 1ull : P0 << 1)) >> lane) & 1u);
    uint32_t ent = 0, v[kScanPer], sum = 0;            // bit i of ent: the state in which the thread's tile i is entered
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        const int64_t t = (int64_t)tid * kScanPer + i;
        ent |= s << i;
        v[i] = t < nt ? (s ? (r[i] >> kCnt1Shift) & kCntMask : r[i] & kCntMask) : 0u;
        sum += v[i];
        s = (r[i] >> (s ? kMap1Bit : kMap0Bit)) & 1u;
    }
    uint32_t inc = sum;                                // inclusive over the wave, then the waves in front
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += t;
    }
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; w++) inc += wsum[w];
    uint32_t run = inc - sum;
#pragma unroll
    for (int i = 0; i < kScanPer; i++) {
        const int64_t t = (int64_t)tid * kScanPer + i;
        if (t < nt) toff[t] = run | ((ent >> i) & 1u) << 31;
        run += v[i];
    }
    if (tid == kScanThreads - 1) {                     // (the tiles behind nt are the identity: s is the state behind the slice)
        *dst = s;
        if (tot) {
            const uint64_t before = first ? 0 : tot[0], total = before + inc;
            if (first) tot[2] = entry;
            tot[1] = before;
            tot[0] = total;
            if (counts_out) {
                counts_out[0] = nelem;
                counts_out[1] = total;
                counts_out[2] = tot[2];
            }
        }
    }
}

// select: stream indices pos0 + i of one tile's transitions, ranked behind tot[1] + toff[tile].  One wave replays the rows; every
// thread then lists the changes of a quarter word as positions inside the tile, in order, in LDS; the indices leave side by side.
__global__ __launch_bounds__(kThreads) void thr_select_kernel(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ rec,
                                                              const uint32_t *__restrict__ toff, const uint64_t *__restrict__ tot, uint64_t pos0,
                                                              uint64_t *__restrict__ idx, uint64_t cap)
{
    __shared__ uint64_t lt[kWords];                    // the changes of every word
    __shared__ uint32_t lbase[kWords];                 // changes of the tile in front of every word
    __shared__ uint16_t lpos[kTile];
    const int64_t tile = blockIdx.x;
    const uint32_t to = toff[tile], e = to >> 31, rc = rec[tile];
    const uint32_t cnt = e ? (rc >> kCnt1Shift) & kCntMask : rc & kCntMask;
    const uint64_t base = tot[1] + (to & kOffMask);
    if (cnt == 0 || base >= cap) return;
    const int tid = threadIdx.x;
    if (tid < kWave) {
        uint64_t S, T;
        replay(mask, tile, tid, e, S, T);
        const uint32_t c = (uint32_t)__popcll(T);
        uint32_t inc = c;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, kWave);
            if (tid >= o) inc += t;
        }
        lt[tid] = T;
        lbase[tid] = inc - c;
    }
    __syncthreads();
    const int w = tid >> 2, q = tid & 3;
    const uint64_t T = lt[w];
    uint32_t bits = (uint32_t)(T >> (16 * q)) & 0xFFFFu;
    uint32_t k = lbase[w] + (uint32_t)__popcll(T & ((1ull << (16 * q)) - 1ull));
    while (bits) {
        lpos[k++] = (uint16_t)(64 * w + 16 * q + __ffs((int)bits) - 1);
        bits &= bits - 1;
    }
    __syncthreads();
    const uint64_t at = pos0 + (uint64_t)tile * kTile;
    for (uint32_t j = tid; j < cnt; j += kThreads)
        if (base + j < cap) idx[base + j] = at + lpos[j];
}

// states: the state after each of the slice's m elements, one byte each
__global__ __launch_bounds__(kWave) void thr_states_kernel(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ toff, int64_t m,
                                                           unsigned char *__restrict__ states)
{
    const int64_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    uint64_t S, T;
    replay(mask, tile, lane, toff[tile] >> 31, S, T);
    const int64_t g0 = tile * kTile + 64 * (int64_t)lane;
#pragma unroll
    for (int b = 0; b < 64; b += 8) {
        const int64_t g = g0 + b;
        uint64_t w = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) w |= ((S >> (b + k)) & 1ull) << (8 * k);
        if (g + 8 <= m) {
            *reinterpret_cast<u64any *>(states + g) = w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (g + k < m) states[g + k] = (unsigned char)(w >> (8 * k));
        }
    }
}

// a call without an element: (0, 0, the carried state)
__global__ void thr_empty_kernel(const uint64_t *carry, uint64_t *tot, uint64_t *counts_out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    tot[0] = tot[1] = 0;
    tot[2] = *carry & 1u;
    counts_out[0] = counts_out[1] = 0;
    counts_out[2] = tot[2];
}

template <typename T>
void classify(const void *in, void *out, size_t m, const ThrShape &p, const ThrWork &w, unsigned nt, hipStream_t st)
{
    T act, deact;
    std::memcpy(&act, p.act, sizeof(T));
    std::memcpy(&deact, p.deact, sizeof(T));
    hipLaunchKernelGGL(thr_classify_kernel<T>, dim3(nt), dim3(kThreads), 0, st, static_cast<const unsigned char *>(in), static_cast<unsigned char *>(out),
                       (int64_t)m, act, deact, w.mask, w.rec);
}

int launch_classify(const ThrShape &p, const void *in, void *out, size_t m, const ThrWork &w, unsigned nt, hipStream_t st)
{
    switch (p.scalar) {
    case PCX_F64: classify<double>(in, out, m, p, w, nt, st); break;
    case PCX_F32: classify<float>(in, out, m, p, w, nt, st); break;
    case PCX_I64: classify<int64_t>(in, out, m, p, w, nt, st); break;
    case PCX_I32: classify<int32_t>(in, out, m, p, w, nt, st); break;
    case PCX_I16: classify<int16_t>(in, out, m, p, w, nt, st); break;
    case PCX_I8: classify<int8_t>(in, out, m, p, w, nt, st); break;
    default: set_error("threshold: unsupported type (scalar %d)", p.scalar); return PCX_ERR_ARG;
    }
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

int check_slice(size_t m)
{
    if (m <= thr_slice()) return PCX_OK;
    set_error("threshold: a slice of %zu elements", m);
    return PCX_ERR_ARG;
}

}  // namespace

size_t thr_tile() { return kTile; }
size_t thr_slice() { return (size_t)1 << kSliceLog; }
size_t thr_mask_words() { return 2 * kWords; }

int launch_thr_empty(const ThrWork &w, uint64_t *counts_out, hipStream_t st)
{
    hipLaunchKernelGGL(thr_empty_kernel, dim3(1), dim3(64), 0, st, (const uint64_t *)w.carry, w.tot, counts_out);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

int launch_thr_slice(const ThrShape &p, const void *in, void *out, size_t m, const ThrWork &w, uint64_t pos0, int first, uint64_t nelem,
                     uint64_t *counts_out, uint64_t *idx, uint64_t cap, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    PCX_TRY(check_slice(m));
    const int64_t nt = (int64_t)((m + kTile - 1) / kTile);
    PCX_TRY(launch_classify(p, in, out, m, w, (unsigned)nt, st));
    hipLaunchKernelGGL(thr_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t *)w.rec, nt, first, (const uint64_t *)w.carry, w.carry, w.tot,
                       w.toff, nelem, counts_out);
    PCX_LAUNCH_CHECK();
    if (cap) {
        hipLaunchKernelGGL(thr_select_kernel, dim3((unsigned)nt), dim3(kThreads), 0, st, (const uint64_t *)w.mask, (const uint32_t *)w.rec,
                           (const uint32_t *)w.toff, (const uint64_t *)w.tot, pos0, idx, cap);
        PCX_LAUNCH_CHECK();
    }
    return PCX_OK;
}

int launch_thr_states(const ThrShape &p, const void *in, size_t m, const ThrWork &w, int first, unsigned char *states, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    PCX_TRY(check_slice(m));
    const int64_t nt = (int64_t)((m + kTile - 1) / kTile);
    PCX_TRY(launch_classify(p, in, nullptr, m, w, (unsigned)nt, st));
    // the carried state is read, never written: the walk over the slices keeps its own word
    hipLaunchKernelGGL(thr_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t *)w.rec, nt, first, (const uint64_t *)(first ? w.carry : w.walk),
                       w.walk, (uint64_t *)nullptr, w.toff, (uint64_t)m, (uint64_t *)nullptr);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL(thr_states_kernel, dim3((unsigned)nt), dim3(kWave), 0, st, (const uint64_t *)w.mask, (const uint32_t *)w.toff, (int64_t)m, states);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace pcx
