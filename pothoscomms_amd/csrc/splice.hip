// splice.hip -- the hot path of /comms/preamble_framer and /comms/frame_insert: a SEGMENTED SPLICE.  The host walks the
// call's labels (frame_plan.hpp) and leaves a table of segments {dst, kind, src}, ascending in dst and in BYTES here; one kernel writes
// the framed stream as one contiguous buffer:
//   INPUT   bytes of the input from src on                      POOL    bytes of the device-resident sync word from src on
//   HEADER  the 58 BPSK header symbols of one frame             ZERO    padding
// A workgroup owns a tile of kTileBytes of output.  It finds the tile's first segment by a wave-uniform binary search over the dst
// offsets and the last one by a gallop from there; while the tile's slice of the table fits kLdsSegs entries it is staged in LDS and
// the lanes search there, beyond that they search global memory between the two bounds.  A lane takes 16-byte units of the output:
//   inside one segment (the hot case)   INPUT, POOL: one 16-byte load at whatever address the source run has, one non-temporal store;
//                                       ZERO: the store alone; HEADER: the symbols made from the frame's bit word and the last preamble
//                                       symbol, bit set +sym, bit clear -sym by flipping the sign bit of each component (the reference's
//                                       unary minus, -0.0 included)
//   across segments                     assembled element by element (byte elements and tiny frames: up to 16 segments in a unit)
// and the unit the output ends in is stored byte by byte.  Exact: every output element is a copy, a zero or a sign flip.  No workgroup
// waits for another; every offset is 64-bit.  The table is trusted: it comes from the planner of the same call and nowhere else.
#include "pcx_internal.hpp"
#include "unit_io.hpp"

namespace pcx {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;
constexpr int kTileBytes = kThreads * kUnroll * 16;       // 16 KiB of output per workgroup
// the longest slice of the table staged in LDS (entries; one more holds the end of the last segment): 8 KiB of LDS, which leaves the
// eight workgroups a compute unit can hold resident
constexpr int kLdsSegs = 511;

constexpr uint64_t kSrcMask = (1ull << 62) - 1;

struct SegRef {
    uint64_t dst, src;      // src: kind << 62 | byte offset (HEADER: index of the bit word)
};

// the entries [lo, hi] of t hold dst <= b for t[lo]: the largest index in [lo, hi] with dst <= b
template <typename P>
__device__ __forceinline__ int64_t seg_find(P t, int64_t lo, int64_t hi, uint64_t b)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (t[mid].dst <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// element k of a header: the last preamble symbol, negated where bit k of the word is clear
template <int ES>
__device__ __forceinline__ void header_elem(uint64_t word, uint32_t k, const uint4 &sym, uint32_t *w)
{
    const uint32_t flip = ((word >> k) & 1ull) ? 0u : 0x80000000u;
    if constexpr (ES == 8) {             // complex_float32: a sign bit per word
        w[0] = sym.x ^ flip;
        w[1] = sym.y ^ flip;
    } else {                             // complex_float64: the sign bit in the high word of each component
        w[0] = sym.x;
        w[1] = sym.y ^ flip;
        w[2] = sym.z;
        w[3] = sym.w ^ flip;
    }
}

template <int ES, bool LDS>
__global__ __launch_bounds__(kThreads) void splice_kernel(const unsigned char *__restrict__ in, const unsigned char *__restrict__ pool,
                                                           const SegRef *__restrict__ segs, int64_t nseg, const uint64_t *__restrict__ headers,
                                                           unsigned char *__restrict__ out, uint64_t total, uint4 sym)
{
    __shared__ SegRef lseg[LDS ? kLdsSegs + 1 : 1];
    const int tid = threadIdx.x;
    const uint64_t b0 = (uint64_t)blockIdx.x * kTileBytes;
    const uint64_t b1 = b0 + kTileBytes < total ? b0 + kTileBytes : total;          // the tile is [b0, b1), not empty
    // segs[nseg] is the sentinel at `total`: s0 and s1 are below it
    const int64_t s0 = seg_find(segs, 0, nseg - 1, b0);
    int64_t hi = s0, step = 1;
    while (hi < nseg - 1 && segs[hi].dst < b1) {              // gallop to an entry at or past the tile's end, or the last one
        hi = hi + step < nseg - 1 ? hi + step : nseg - 1;
        step *= 2;
    }
    const int64_t s1 = seg_find(segs, s0, hi, b1 - 1);
    const bool staged = LDS && s1 - s0 < kLdsSegs;
    if (staged) {
        for (int64_t k = tid; k <= s1 - s0 + 1; k += kThreads) lseg[k] = segs[s0 + k];
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < kUnroll; r++) {
        const uint64_t b = b0 + 16 * (uint64_t)(r * kThreads + tid);
        if (b >= total) continue;
        int64_t s;
        SegRef cur;
        uint64_t next;
        if (staged) {
            s = seg_find(lseg, 0, s1 - s0, b);
            cur = lseg[s];
            next = lseg[s + 1].dst;
        } else {
            s = seg_find(segs, s0, s1, b);
            cur = segs[s];
            next = segs[s + 1].dst;
        }
        if (next >= b + 16) {              // the unit lies inside one segment (and inside the output: next <= total)
            const uint32_t kind = (uint32_t)(cur.src >> 62);
            const uint64_t off = (cur.src & kSrcMask) + (b - cur.dst);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (kind == 0) v = nt_load16_any(in + off);
            else if (kind == 1) v = nt_load16_any(pool + off);
            else if (kind == 2) {
                if constexpr (ES > 1) {
                    const uint64_t word = headers[cur.src & kSrcMask];
                    const uint32_t k = (uint32_t)((b - cur.dst) / ES);
                    uint32_t w[4];
                    header_elem<ES>(word, k, sym, w);
                    if constexpr (ES == 8) header_elem<ES>(word, k + 1, sym, w + 2);
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
            nt_store16_any(out + b, v);
            continue;
        }
        // the unit crosses a boundary: element by element, walking the table forward
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16 / ES; j++) {
            const uint64_t p = b + (uint64_t)j * ES;
            if (p < total) {
                while (next <= p) {
                    s++;
                    if (staged) {
                        cur = lseg[s];
                        next = lseg[s + 1].dst;
                    } else {
                        cur = segs[s];
                        next = segs[s + 1].dst;
                    }
                }
                const uint32_t kind = (uint32_t)(cur.src >> 62);
                const uint64_t off = (cur.src & kSrcMask) + (p - cur.dst);
                if constexpr (ES == 1) {
                    uint32_t e = 0;
                    if (kind == 0) e = in[off];
                    else if (kind == 1) e = pool[off];
                    w[j >> 2] |= e << (8 * (j & 3));
                } else {
                    typedef uint32_t __attribute__((aligned(1), may_alias)) u32any;
                    uint32_t e[ES / 4];
#pragma unroll
                    for (int q = 0; q < ES / 4; q++) e[q] = 0;
                    if (kind == 0 || kind == 1) {
                        const u32any *src = reinterpret_cast<const u32any *>((kind == 0 ? in : pool) + off);
#pragma unroll
                        for (int q = 0; q < ES / 4; q++) e[q] = src[q];
                    } else if (kind == 2) {
                        header_elem<ES>(headers[cur.src & kSrcMask], (uint32_t)((p - cur.dst) / ES), sym, e);
                    }
#pragma unroll
                    for (int q = 0; q < ES / 4; q++) w[j * (ES / 4) + q] = e[q];
                }
            }
        }
        store_unit(out, (int64_t)b, (int64_t)total, make_uint4(w[0], w[1], w[2], w[3]));
    }
}

template <int ES>
int launch_es(bool lds, const void *in, const void *pool, const void *segs, size_t nseg, const void *headers, void *out, size_t total, const uint4 &sym,
              hipStream_t st)
{
    const uint64_t tiles = ((uint64_t)total + kTileBytes - 1) / kTileBytes;
    if (tiles > 0x7fffffffull) {
        set_error("framer: %zu output bytes in one call", total);
        return PCX_ERR_ARG;
    }
    auto k = lds ? splice_kernel<ES, true> : splice_kernel<ES, false>;
    hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(kThreads), 0, st, static_cast<const unsigned char *>(in), static_cast<const unsigned char *>(pool),
                       static_cast<const SegRef *>(segs), (int64_t)nseg, static_cast<const uint64_t *>(headers), static_cast<unsigned char *>(out),
                       (uint64_t)total, sym);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace

size_t splice_tile_bytes() { return kTileBytes; }
size_t splice_lds_segments() { return kLdsSegs; }

// total output bytes from a table of nseg segments and the sentinel behind them (SpliceSeg: dst in bytes, src = kind << 62 | bytes);
// sym: the 16 bytes (complex_float32: the first 8) of the last preamble symbol
int launch_splice(size_t es, const void *in, const void *pool, const SpliceSeg *segs, size_t nseg, const uint64_t *headers, void *out, size_t total,
                  const unsigned char sym[16], hipStream_t st)
{
    static_assert(sizeof(SpliceSeg) == sizeof(SegRef), "the table as the kernel reads it");
    if (!total) return PCX_OK;
    if (!nseg) {
        set_error("framer: %zu output bytes without a segment", total);
        return PCX_ERR_ARG;
    }
    uint4 s;
    std::memcpy(&s, sym, 16);
    // the diagnostic build's A/B switch: search global memory in every tile
    const bool lds = !PCX_ENV_SET("PCX_FRM_NO_LDS");
    switch (es) {
    case 1: return launch_es<1>(lds, in, pool, segs, nseg, headers, out, total, s, st);
    case 8: return launch_es<8>(lds, in, pool, segs, nseg, headers, out, total, s, st);
    case 16: return launch_es<16>(lds, in, pool, segs, nseg, headers, out, total, s, st);
    }
    set_error("framer: elements of %zu bytes", es);
    return PCX_ERR_ARG;
}

}  // namespace pcx
