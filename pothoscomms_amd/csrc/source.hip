// source.hip -- the two blocks that produce a stream:
//   /comms/waveform_source   waveform/WaveformSource.cpp:98-108   out[i] = table[index & mask]; index += step
//   /comms/noise_source      waveform/NoiseSource.cpp:109-117     index += draw; out[i] = table[index % 4096]; index++
// Both walk a table of the output type cyclically from a carried index: out[i] = table[(index + i * step) & (size - 1)], modulo 2^64.
// The outputs are table entries, copied and never computed, so every output is the reference's bit for bit.
//
// THE PERIOD, not the stride.  With g = gcd(step mod size, size) the stream repeats after P = size / g elements, a power of two (a
// step that is a multiple of the size gives P = 1).  Two kernels:
//   permute      seq[j] = table[(index0 + j * step) & mask] for the P elements of one period: the strided gather, paid once per table,
//                step or index that was SET (a call's own advance is not one), never per sample.  The period is written out to at
//                least 16 bytes and 16 bytes past its end, so that a 16-byte read may start at any of its bytes.
//   wrapped copy out = the bytes of seq from the call's phase on, cyclically.  The element size is gone here: the stream is bytes with
//                a period of PB = max(P * es, 16) bytes, a power of two.  The bytes in front of the first 16-byte boundary of `out` and
//                behind the last go one by one (workgroup 0); between them every lane stores aligned 16-byte units with the
//                non-temporal hint, lanes side by side, unit u from byte (r + 16 u) & (PB - 1) of the period (r: the phase at the first
//                unit).  While PB fits kLdsBytes a workgroup first stages the period ROTATED by r in LDS, so that unit u is the aligned
//                entry u & (PB / 16 - 1): consecutive lanes read consecutive 16-byte entries, which is free of bank conflicts, and every
//                workgroup stages the same image whatever tiles it walks.  A longer period is read from global memory in the same
//                pattern (coalesced, at any byte offset; the 16 bytes past the end take the wrap).
// A workgroup's tile is kBlock * kUnroll units (16 KiB of output), a multiple of every staged period's units.  No workgroup waits for
// another; every index is 64-bit.  The diagnostic build (-DPCX_DIAG) also holds the plain per-element gather, the A/B partner.
#include <algorithm>

#include "pcx_internal.hpp"
#include "vec_io.hpp"

namespace pcx {
namespace {

constexpr int kBlock = 256;
constexpr int kUnroll = 4;
constexpr size_t kTileUnits = (size_t)kBlock * kUnroll;     // 16-byte units per workgroup and pass
// the longest period staged in LDS.  Measured (tools/source_rate.py, profiles/source/): against reading the same period from global
// memory, staging wins 1.7 % at 8 KiB, ties at 16 KiB and loses 6 to 8 % at 16 and 32 KiB on calls of 512 MiB and more
constexpr size_t kLdsBytes = 8u << 10;
constexpr unsigned kLdsGrid = 256 * 8;                      // workgroups of a staged launch: each stages once and walks many tiles
constexpr unsigned kGlobalGrid = 256 * 64;

typedef RawVec<16>::type Raw16;
typedef Raw16 Raw16Any __attribute__((aligned(1)));         // gfx950 takes unaligned global accesses at full width (repack.hip)

template <int ES>
__global__ __launch_bounds__(kBlock) void source_permute_kernel(const unsigned char *__restrict__ table, unsigned char *__restrict__ seq,
                                                                 uint64_t index, uint64_t step, uint64_t mask, uint64_t count)
{
    typedef typename RawVec<ES>::type E;
    const E *t = reinterpret_cast<const E *>(table);
    E *s = reinterpret_cast<E *>(seq);
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < count; j += (uint64_t)gridDim.x * kBlock) s[j] = t[(index + j * step) & mask];
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void source_copy_kernel(const unsigned char *__restrict__ seq, unsigned char *__restrict__ out, uint64_t nbytes,
                                                              uint64_t phase, uint64_t pmask)
{
    extern __shared__ Raw16 img[];
    const uint64_t tid = threadIdx.x;
    const uint64_t gap = (16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15;
    const uint64_t head = gap < nbytes ? gap : nbytes;
    const uint64_t units = (nbytes - head) >> 4;
    const uint64_t r = (phase + head) & pmask;
    if constexpr (LDS) {
        for (uint64_t v = tid; v <= (pmask >> 4); v += kBlock) img[v] = *reinterpret_cast<const Raw16Any *>(seq + ((r + 16 * v) & pmask));
        __syncthreads();
    }
    Raw16 *o = reinterpret_cast<Raw16 *>(out + head);
    const uint64_t umask = pmask >> 4;
    for (uint64_t base = (uint64_t)blockIdx.x * kTileUnits; base < units; base += (uint64_t)gridDim.x * kTileUnits) {
#pragma unroll
        for (int k = 0; k < kUnroll; k++) {
            const uint64_t u = base + (uint64_t)k * kBlock + tid;
            if (u < units) {
                Raw16 v;
                if constexpr (LDS) v = img[u & umask];
                else v = *reinterpret_cast<const Raw16Any *>(seq + ((r + 16 * u) & pmask));
                __builtin_nontemporal_store(v, o + u);
            }
        }
    }
    if (blockIdx.x == 0) {
        for (uint64_t b = tid; b < head; b += kBlock) out[b] = seq[(phase + b) & pmask];
        for (uint64_t b = head + 16 * units + tid; b < nbytes; b += kBlock) out[b] = seq[(phase + b) & pmask];
    }
}

#ifdef PCX_DIAG
// the plain form: one element per lane and step, read where the walk stands (diagnostic build only)
template <int ES>
__global__ __launch_bounds__(kBlock) void source_gather_kernel(const unsigned char *__restrict__ table, unsigned char *__restrict__ out, uint64_t index,
                                                                uint64_t step, uint64_t mask, uint64_t n)
{
    typedef typename RawVec<ES>::type E;
    typedef E EAny __attribute__((aligned(1)));     // a complex_float64 stream is 8-byte aligned
    const E *t = reinterpret_cast<const E *>(table);
    EAny *o = reinterpret_cast<EAny *>(out);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
        __builtin_nontemporal_store(t[(index + i * step) & mask], o + i);
}
#endif

typedef void (*TableKernel)(const unsigned char *, unsigned char *, uint64_t, uint64_t, uint64_t, uint64_t);
template <template <int> class K>
TableKernel pick_es(size_t es)
{
    switch (es) {
    case 1: return K<1>::fn();
    case 2: return K<2>::fn();
    case 4: return K<4>::fn();
    case 8: return K<8>::fn();
    case 16: return K<16>::fn();
    }
    return nullptr;
}
template <int ES> struct Permute { static TableKernel fn() { return source_permute_kernel<ES>; } };
#ifdef PCX_DIAG
template <int ES> struct Gather { static TableKernel fn() { return source_gather_kernel<ES>; } };
#endif

unsigned grid_for(uint64_t items, uint64_t per_block, unsigned cap)
{
    if (g_link_map_grid) cap = g_link_map_grid;
    const uint64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace

size_t source_tile_bytes() { return kTileUnits * 16; }
size_t source_lds_bytes() { return kLdsBytes; }
size_t source_max_entries() { return (size_t)1 << 20; }
// bytes of seq for a period of `period` elements of `es` bytes: the period written out to at least 16 bytes, and 16 bytes more
size_t source_seq_bytes(size_t period, size_t es) { return std::max<size_t>(period * es, 16) + 16; }

int launch_source_permute(size_t es, const void *table, void *seq, uint64_t index, uint64_t step, size_t entries, size_t period, hipStream_t st)
{
    TableKernel k = pick_es<Permute>(es);
    if (!k || !entries || (entries & (entries - 1)) || entries > source_max_entries() || period > entries) {
        set_error("source: %zu entries of %zu bytes, period %zu", entries, es, period);
        return PCX_ERR_ARG;
    }
    const uint64_t count = source_seq_bytes(period, es) / es;
    hipLaunchKernelGGL(k, dim3(grid_for(count, kBlock, kGlobalGrid)), dim3(kBlock), 0, st, static_cast<const unsigned char *>(table),
                       static_cast<unsigned char *>(seq), index, step, (uint64_t)entries - 1, count);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

// nbytes of output from byte `phase` of the period on; period_bytes: a power of two of at least 16, seq holds 16 bytes more
int launch_source_copy(const void *seq, void *out, size_t nbytes, size_t phase, size_t period_bytes, hipStream_t st)
{
    if (nbytes == 0) return PCX_OK;
    if (period_bytes < 16 || (period_bytes & (period_bytes - 1)) || phase >= period_bytes) {
        set_error("source: a period of %zu bytes, phase %zu", period_bytes, phase);
        return PCX_ERR_ARG;
    }
    const bool lds = period_bytes <= kLdsBytes && !PCX_ENV_SET("PCX_SRC_NO_LDS");
    const unsigned grid = grid_for(nbytes / 16, kTileUnits, lds ? kLdsGrid : kGlobalGrid);
    if (lds)
        hipLaunchKernelGGL(source_copy_kernel<true>, dim3(grid), dim3(kBlock), period_bytes, st, static_cast<const unsigned char *>(seq),
                           static_cast<unsigned char *>(out), (uint64_t)nbytes, (uint64_t)phase, (uint64_t)period_bytes - 1);
    else
        hipLaunchKernelGGL(source_copy_kernel<false>, dim3(grid), dim3(kBlock), 0, st, static_cast<const unsigned char *>(seq),
                           static_cast<unsigned char *>(out), (uint64_t)nbytes, (uint64_t)phase, (uint64_t)period_bytes - 1);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

// the diagnostic build's per-element gather when PCX_SRC_GATHER is set there; the product has none
bool source_gather_selected() { return PCX_ENV_SET("PCX_SRC_GATHER"); }
int launch_source_gather(size_t es, const void *table, void *out, uint64_t index, uint64_t step, size_t entries, size_t n, hipStream_t st)
{
#ifdef PCX_DIAG
    TableKernel k = pick_es<Gather>(es);
    if (!k || !entries || (entries & (entries - 1))) {
        set_error("source gather: %zu entries of %zu bytes", entries, es);
        return PCX_ERR_ARG;
    }
    if (n == 0) return PCX_OK;
    hipLaunchKernelGGL(k, dim3(grid_for(n, kBlock, kGlobalGrid)), dim3(kBlock), 0, st, static_cast<const unsigned char *>(table),
                       static_cast<unsigned char *>(out), index, step, (uint64_t)entries - 1, (uint64_t)n);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
#else
    set_error("source gather: diagnostic build only");
    return PCX_ERR_UNSUPPORTED;
#endif
}

}  // namespace pcx
