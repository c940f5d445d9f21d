// trigger.hip -- /comms/wave_trigger (utility/WaveTrigger.cpp:735-771, :515-582): the level search and the window capture.
//
// SEARCH.  Element k of the stream becomes a float y[k]: static_cast<float> of a real element, and of a complex one the modulus of the
// converted components (std::abs(std::complex<float>) = glibc's hypotf, elementwise.hip's AbsCplxF32).  Pair i = (y[i], y[i + 1])
// TRIGGERS when y0 < level && y1 >= level (POS), y0 > level && y1 <= level (NEG) or either (LEVEL), compared in double: a NaN never
// does.  Wanted is the LEAST triggering i in [from, n - 2].
//   Pairs are cut into tiles of kTile; workgroup b takes the tiles b, b + G, b + 2 G ... of the range in ascending order.  A wave owns
//   64 consecutive pairs at a time: a lane converts its own element once, takes its neighbour's from the next lane (the last lane of a
//   wave reads the one element of halo) and the wave's first triggering lane -- the lowest set bit of a 64-lane ballot -- offers its
//   index to one 64-bit word with atomicMin.  A wave that found a pair is done (its later pairs are larger); a wave whose next pairs
//   begin behind the word's value is done too.  Nobody waits for anybody, and the word ends at the minimum whatever the order of
//   arrival.  A second launch of one thread reads the word and leaves (found, i, y0, y1): the host forms i + (level - y0) / (y1 - y0)
//   from them with the reference's own roundings (a float subtraction, the rest double).
// CAPTURE.  Rows [starts[e], starts[e] + W) of every port into an nev x W matrix per port, in 16-byte units at any byte address
// (unit_io.hpp), all ports in one launch.
#include "pcx_internal.hpp"
#include "unit_io.hpp"

namespace pcx {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kPer = 8;                               // rounds of a workgroup over a tile
constexpr int64_t kTile = (int64_t)kThreads * kPer;   // pairs of a tile
constexpr unsigned kMaxGrid = 2048;                   // 256 compute units x 8 resident workgroups
constexpr uint64_t kNone = ~(uint64_t)0;

// element k of the stream as the float the reference searches (WaveTrigger.cpp:737, :756, :761)
template <typename S, bool CPLX>
__device__ __forceinline__ float as_search_float(const unsigned char *in, int64_t k)
{
    if constexpr (CPLX) {
        S s[2];
        __builtin_memcpy(s, in + k * (int64_t)(2 * sizeof(S)), 2 * sizeof(S));
        const float a = static_cast<float>(s[0]), b = static_cast<float>(s[1]);
        if (isinf(a) || isinf(b)) return INFINITY;    // hypotf (glibc 2.35): (float)sqrt((double)a*a + (double)b*b) behind the inf cases
        const double da = (double)a, db = (double)b;
        return (float)sqrt(da * da + db * db);
    } else {
        S s;
        __builtin_memcpy(&s, in + k * (int64_t)sizeof(S), sizeof(S));
        return static_cast<float>(s);
    }
}

__device__ __forceinline__ bool triggers(float y0, float y1, double level, int slope)
{
    const double a = (double)y0, b = (double)y1;
    const bool pos = a < level && b >= level, neg = a > level && b <= level;
    return slope == PCX_TRIGGER_POS ? pos : slope == PCX_TRIGGER_NEG ? neg : (pos || neg);
}

// pairs from .. last (last = n - 2) of the n elements at `in`; *best arrives as kNone and leaves as the least triggering pair
template <typename S, bool CPLX>
__global__ __launch_bounds__(kThreads) void trigger_search_kernel(const unsigned char *__restrict__ in, int64_t n, int64_t from, int64_t ntiles, double level,
                                                                  int slope, unsigned long long *best)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int64_t last = n - 2;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t p0 = from + t * kTile;          // the tile's first pair
        for (int r = 0; r < kPer; r++) {
            // the wave's 64 pairs of this round begin at w0: the same in every lane, and so is everything the loop branches on
            const int64_t w0 = p0 + (int64_t)r * kThreads + (int64_t)wave * kWave;
            const unsigned long long load = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long seen = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(load >> 32)) << 32) |
                                            (unsigned)__builtin_amdgcn_readfirstlane((int)load);
            if (w0 > last || (unsigned long long)w0 > seen) return;     // every later pair of this wave is larger still
            const int64_t i = w0 + lane;
            const float y0 = i < n ? as_search_float<S, CPLX>(in, i) : 0.0f;
            float y1 = __shfl_down(y0, 1, kWave);     // all 64 lanes are here: the branches above are the wave's
            if (lane == kWave - 1 && i + 1 < n) y1 = as_search_float<S, CPLX>(in, i + 1);
            const bool hit = i <= last && triggers(y0, y1, level, slope);
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                if (lane == __ffsll((long long)mask) - 1) atomicMin(best, (unsigned long long)i);
                return;
            }
        }
    }
}

// what the host needs of the winner: 24 bytes
struct Found {
    uint64_t i;
    float y0, y1;
    uint64_t found;
};
template <typename S, bool CPLX>
__global__ void trigger_finish_kernel(const unsigned char *__restrict__ in, const unsigned long long *best, Found *out)
{
    const unsigned long long b = *best;
    Found f;
    f.found = b != kNone;
    f.i = f.found ? b : 0;
    f.y0 = f.found ? as_search_float<S, CPLX>(in, (int64_t)b) : 0.0f;
    f.y1 = f.found ? as_search_float<S, CPLX>(in, (int64_t)b + 1) : 0.0f;
    *out = f;
}
__global__ void trigger_none_kernel(Found *out)
{
    Found f;
    f.i = 0; f.y0 = f.y1 = 0.0f; f.found = 0;
    *out = f;
}

template <typename S, bool CPLX>
int search(const void *in, size_t n, size_t from, double level, int slope, uint64_t *best, void *result, hipStream_t st)
{
    const int64_t npairs = (int64_t)n - 1 - (int64_t)from, ntiles = (npairs + kTile - 1) / kTile;
    PCX_HIP(hipMemsetAsync(best, 0xFF, sizeof(uint64_t), st));
    const unsigned grid = (unsigned)std::min<int64_t>(ntiles, kMaxGrid);
    hipLaunchKernelGGL((trigger_search_kernel<S, CPLX>), dim3(grid), dim3(kThreads), 0, st, static_cast<const unsigned char *>(in), (int64_t)n, (int64_t)from,
                       ntiles, level, slope, reinterpret_cast<unsigned long long *>(best));
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((trigger_finish_kernel<S, CPLX>), dim3(1), dim3(1), 0, st, static_cast<const unsigned char *>(in),
                       reinterpret_cast<const unsigned long long *>(best), static_cast<Found *>(result));
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}
template <typename S>
int search_kind(bool cplx, const void *in, size_t n, size_t from, double level, int slope, uint64_t *best, void *result, hipStream_t st)
{
    return cplx ? search<S, true>(in, n, from, level, slope, best, result, st) : search<S, false>(in, n, from, level, slope, best, result, st);
}

// ---- capture ----
constexpr int kCapUnits = 4;                          // 16-byte units a thread moves per round
struct CapPorts {
    const unsigned char *in[PCX_TRIGGER_MAX_PORTS];
    unsigned char *out[PCX_TRIGGER_MAX_PORTS];
    uint32_t es[PCX_TRIGGER_MAX_PORTS];
};
// workgroup (x, e, p): chunk x of row e of port p; a row is W es[p] bytes from byte starts[e] es[p] of the port's buffer
__global__ __launch_bounds__(kThreads) void trigger_capture_kernel(CapPorts ports, const uint64_t *__restrict__ starts, int64_t W)
{
    const int p = blockIdx.z;
    const int64_t e = blockIdx.y, es = ports.es[p], row = W * es;
    const unsigned char *src = ports.in[p] + (int64_t)starts[e] * es;
    unsigned char *dst = ports.out[p] + e * row;
    const int64_t chunk = (int64_t)kThreads * kCapUnits * 16;
    for (int64_t c = (int64_t)blockIdx.x * chunk; c < row; c += (int64_t)gridDim.x * chunk) {
        uint4 v[kCapUnits];
#pragma unroll
        for (int u = 0; u < kCapUnits; u++) {
            const int64_t off = c + ((int64_t)u * kThreads + threadIdx.x) * 16;
            if (off < row) v[u] = load_unit(src, off, row);
        }
#pragma unroll
        for (int u = 0; u < kCapUnits; u++) {
            const int64_t off = c + ((int64_t)u * kThreads + threadIdx.x) * 16;
            if (off < row) store_unit(dst, off, row, v[u]);
        }
    }
}

}  // namespace

size_t trigger_tile() { return (size_t)kTile; }

int launch_trigger_search(int scalar, bool cplx, const void *in, size_t n, size_t from, double level, int slope, uint64_t *best, void *result, hipStream_t st)
{
    if (n < 2 || from > n - 2) {                      // no pair in the range
        hipLaunchKernelGGL(trigger_none_kernel, dim3(1), dim3(1), 0, st, static_cast<Found *>(result));
        PCX_LAUNCH_CHECK();
        return PCX_OK;
    }
    switch (scalar) {
    case PCX_F64: return search_kind<double>(cplx, in, n, from, level, slope, best, result, st);
    case PCX_F32: return search_kind<float>(cplx, in, n, from, level, slope, best, result, st);
    case PCX_I64: return search_kind<int64_t>(cplx, in, n, from, level, slope, best, result, st);
    case PCX_I32: return search_kind<int32_t>(cplx, in, n, from, level, slope, best, result, st);
    case PCX_I16: return search_kind<int16_t>(cplx, in, n, from, level, slope, best, result, st);
    case PCX_I8: return search_kind<int8_t>(cplx, in, n, from, level, slope, best, result, st);
    }
    if (!cplx) switch (scalar) {
    case PCX_U64: return search<uint64_t, false>(in, n, from, level, slope, best, result, st);
    case PCX_U32: return search<uint32_t, false>(in, n, from, level, slope, best, result, st);
    case PCX_U16: return search<uint16_t, false>(in, n, from, level, slope, best, result, st);
    case PCX_U8: return search<uint8_t, false>(in, n, from, level, slope, best, result, st);
    }
    set_error("wave trigger: unsupported type (scalar %d%s)", scalar, cplx ? ", complex" : "");
    return PCX_ERR_ARG;
}

int launch_trigger_capture(size_t nports, const void *const *ins, const size_t *elem_bytes, const uint64_t *starts, size_t nev, size_t W, void *const *outs,
                           hipStream_t st)
{
    if (!nports || !nev || !W) return PCX_OK;
    CapPorts ports = {};
    size_t widest = 0;
    for (size_t p = 0; p < nports; p++) {
        ports.in[p] = static_cast<const unsigned char *>(ins[p]);
        ports.out[p] = static_cast<unsigned char *>(outs[p]);
        ports.es[p] = (uint32_t)elem_bytes[p];
        widest = std::max(widest, W * elem_bytes[p]);
    }
    const size_t chunk = (size_t)kThreads * kCapUnits * 16;
    const unsigned gx = (unsigned)std::min<size_t>((widest + chunk - 1) / chunk, 1024);
    for (size_t e0 = 0; e0 < nev; e0 += 65535) {      // (the y dimension of a grid)
        const size_t take = std::min<size_t>(nev - e0, 65535);
        CapPorts part = ports;
        for (size_t p = 0; p < nports; p++) part.out[p] += e0 * W * elem_bytes[p];
        hipLaunchKernelGGL(trigger_capture_kernel, dim3(gx, (unsigned)take, (unsigned)nports), dim3(kThreads), 0, st, part, starts + e0, (int64_t)W);
        PCX_LAUNCH_CHECK();
    }
    return PCX_OK;
}

}  // namespace pcx
