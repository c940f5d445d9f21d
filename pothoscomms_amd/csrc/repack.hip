// repack.hip -- the four blocks that join bits, symbols and payload bytes:
//   /comms/bits_to_symbols    digital/SymbolHelpers.hpp:13-41     W one-bit bytes (a byte counts as 1 when it is not 0) -> one symbol
//   /comms/symbols_to_bits    digital/SymbolHelpers.hpp:46-72     the low W bits of a symbol -> W bytes of 0 / 1
//   /comms/bytes_to_symbols   digital/SymbolHelpers.hpp:233-414   W bytes -> eight symbols below 2^W
//   /comms/symbols_to_bytes   digital/SymbolHelpers.hpp:77-228    eight symbols -> W bytes, by the clipped OR (repack_core.hpp)
// Every output byte equals the reference's loop for all 256 values of every input byte.  Nothing is carried between calls.
//
// ONE SHAPE for the 64 instantiations (kind x W x order are template parameters, every shift and mask a constant).  A workgroup's
// tile is 8192 symbols; between the symbols and the 1024 W bytes that hold them stands the PACKED stream, which for the two byte
// kinds is the input resp. the output itself and for the two bit kinds an intermediate that never leaves the chip:
//   to symbols    packed bytes into LDS | every lane takes its 4 W bytes (W words), extracts 32 symbols, leaves them in LDS | stored
//   from symbols  symbols into LDS | every lane takes its 32, packs them into W words, leaves them in LDS | the packed bytes stored
//   bits          a lane turns each 16-byte unit of one-bit bytes into 2 bytes of the packed stream on the way in (the != 0 test on
//                 eight bytes at once, four flags gathered by one multiplication) and each 2 bytes into a unit on the way out
// Both sides of a tile therefore move as 16-byte units, lanes side by side (unit u of round k is lane u - 256 k's), with the
// non-temporal hint, whatever W is: the odd ratios are met in LDS, where a lane's W words sit at word W * lane (W odd: no two lanes of
// a half wave on one bank; W even: up to 8 on one, at an LDS traffic below a tenth of what the array moves per clock at the HBM rate).
// The units are addressed from byte pointers, so they hold at any alignment of either buffer; the units of a tile that the call ends
// in go byte by byte.  A call is whole groups, so every byte a produced output depends on lies inside the call.
// No workgroup waits for another, every index is 64-bit.
#include "pcx_internal.hpp"
#include "repack_core.hpp"
#include "unit_io.hpp"

namespace pcx {
namespace {

using namespace repack;

constexpr int kBlock = 256;
constexpr int kTileSyms = kBlock * 32;          // symbols per workgroup
constexpr int kSymUnits = kTileSyms / 16;
constexpr int kSliceLog = 26;                   // a call slice is the largest whole number of tiles within 2^26 input elements

template <int KIND, int W>
struct Tile {
    static constexpr bool kToSyms = KIND == PCX_REPACK_BITS_TO_SYMBOLS || KIND == PCX_REPACK_BYTES_TO_SYMBOLS;
    static constexpr bool kBits = KIND == PCX_REPACK_BITS_TO_SYMBOLS || KIND == PCX_REPACK_SYMBOLS_TO_BITS;
    static constexpr int kPackedUnits = kTileSyms * W / 8 / 16;         // 64 W
    static constexpr int64_t kOther = kBits ? (int64_t)kTileSyms * W : (int64_t)kTileSyms * W / 8;       // bytes of the side that is not symbols
    static constexpr int64_t kIn = kToSyms ? kOther : kTileSyms, kOut = kToSyms ? kTileSyms : kOther;
};

template <int KIND, int W, bool MSB>
__global__ __launch_bounds__(kBlock) void repack_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, int64_t n_in,
                                                         int64_t n_out)
{
    typedef Tile<KIND, W> G;
    __shared__ uint4 packed[G::kPackedUnits];
    __shared__ uint4 syms[kSymUnits];
    uint32_t *pw = reinterpret_cast<uint32_t *>(packed) + W * threadIdx.x;      // the lane's W words
    unsigned short *p16 = reinterpret_cast<unsigned short *>(packed);
    const int tid = threadIdx.x;
    const int64_t ntiles = (n_in + G::kIn - 1) / G::kIn;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t i0 = t * G::kIn, o0 = t * G::kOut;
        if constexpr (G::kToSyms) {
            if constexpr (G::kBits) {
#pragma unroll
                for (int k = 0; k < 2 * W; k++) {
                    const int u = k * kBlock + tid;
                    const uint4 v = load_unit(in, i0 + 16 * (int64_t)u, n_in);
                    p16[u] = (unsigned short)gather16<MSB>((uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32));
                }
            } else {
                for (int u = tid; u < G::kPackedUnits; u += kBlock) packed[u] = load_unit(in, i0 + 16 * (int64_t)u, n_in);
            }
            __syncthreads();
            uint32_t p[W], s[8];
#pragma unroll
            for (int i = 0; i < W; i++) p[i] = pw[i];
            extract32<W, MSB>(p, s);
            syms[2 * tid] = make_uint4(s[0], s[1], s[2], s[3]);
            syms[2 * tid + 1] = make_uint4(s[4], s[5], s[6], s[7]);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kSymUnits / kBlock; k++) {
                const int u = k * kBlock + tid;
                store_unit(out, o0 + 16 * (int64_t)u, n_out, syms[u]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kSymUnits / kBlock; k++) {
                const int u = k * kBlock + tid;
                syms[u] = load_unit(in, i0 + 16 * (int64_t)u, n_in);
            }
            __syncthreads();
            const uint4 a = syms[2 * tid], b = syms[2 * tid + 1];
            const uint32_t s[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t p[W];
            pack32<W, MSB, G::kBits>(s, p);         // the bit kind looks at the low W bits only
#pragma unroll
            for (int i = 0; i < W; i++) pw[i] = p[i];
            __syncthreads();
            if constexpr (G::kBits) {
#pragma unroll
                for (int k = 0; k < 2 * W; k++) {
                    const int u = k * kBlock + tid;
                    uint32_t o[4];
                    spread16<MSB>(p16[u], o);
                    store_unit(out, o0 + 16 * (int64_t)u, n_out, make_uint4(o[0], o[1], o[2], o[3]));
                }
            } else {
                for (int u = tid; u < G::kPackedUnits; u += kBlock) store_unit(out, o0 + 16 * (int64_t)u, n_out, packed[u]);
            }
        }
        // (the next tile's first writes into an array come behind a barrier that follows this tile's last reads of it)
    }
}

typedef void (*Kernel)(const unsigned char *, unsigned char *, int64_t, int64_t);
template <int KIND, int W>
Kernel pick_order(bool msb) { return msb ? repack_kernel<KIND, W, true> : repack_kernel<KIND, W, false>; }
template <int KIND>
Kernel pick_width(unsigned w, bool msb)
{
    switch (w) {
    case 1: return pick_order<KIND, 1>(msb);
    case 2: return pick_order<KIND, 2>(msb);
    case 3: return pick_order<KIND, 3>(msb);
    case 4: return pick_order<KIND, 4>(msb);
    case 5: return pick_order<KIND, 5>(msb);
    case 6: return pick_order<KIND, 6>(msb);
    case 7: return pick_order<KIND, 7>(msb);
    case 8: return pick_order<KIND, 8>(msb);
    }
    return nullptr;
}

}  // namespace

size_t repack_tile(int kind, unsigned w)
{
    switch (kind) {
    case PCX_REPACK_BITS_TO_SYMBOLS: return (size_t)kTileSyms * w;
    case PCX_REPACK_BYTES_TO_SYMBOLS: return (size_t)kTileSyms * w / 8;
    }
    return kTileSyms;
}
size_t repack_slice(int kind, unsigned w)
{
    const size_t tile = repack_tile(kind, w);
    return (((size_t)1 << kSliceLog) / tile) * tile;
}
size_t repack_out_elems(int kind, unsigned w, size_t in_elems)
{
    switch (kind) {
    case PCX_REPACK_BITS_TO_SYMBOLS: return in_elems / w;
    case PCX_REPACK_SYMBOLS_TO_BITS: return in_elems * w;
    case PCX_REPACK_BYTES_TO_SYMBOLS: return in_elems * 8 / w;
    }
    return in_elems * w / 8;
}

int launch_repack_slice(int kind, unsigned w, bool msb, const void *in, void *out, size_t m, hipStream_t st)
{
    if (m == 0) return PCX_OK;
    Kernel k = nullptr;
    switch (kind) {
    case PCX_REPACK_BITS_TO_SYMBOLS: k = pick_width<PCX_REPACK_BITS_TO_SYMBOLS>(w, msb); break;
    case PCX_REPACK_SYMBOLS_TO_BITS: k = pick_width<PCX_REPACK_SYMBOLS_TO_BITS>(w, msb); break;
    case PCX_REPACK_BYTES_TO_SYMBOLS: k = pick_width<PCX_REPACK_BYTES_TO_SYMBOLS>(w, msb); break;
    case PCX_REPACK_SYMBOLS_TO_BYTES: k = pick_width<PCX_REPACK_SYMBOLS_TO_BYTES>(w, msb); break;
    }
    if (!k || m > repack_slice(kind, w)) {
        set_error("repack: kind %d, modulus %u, a slice of %zu elements", kind, w, m);
        return PCX_ERR_ARG;
    }
    const size_t tile = repack_tile(kind, w);
    const unsigned grid = stream_grid(((m + tile - 1) / tile) * kBlock, kBlock);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, st, static_cast<const unsigned char *>(in), static_cast<unsigned char *>(out), (int64_t)m,
                       (int64_t)repack_out_elems(kind, w, m));
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace pcx
