// unit_io.hpp -- 16-byte units at ANY byte address, with the non-temporal hint of vec_io.hpp and a byte-wise path for the unit a
// buffer ends in (repack.hip, threshold.hip).
#pragma once
#include <cstdint>

#include "vec_io.hpp"

namespace pcx {

// 16 bytes at ANY byte address with the non-temporal hint of vec_io.hpp: gfx950 takes unaligned global accesses at full width, the
// type only has to say that nothing is promised about the address (global_load_dwordx4 ... nt / global_store_dwordx4 ... nt)
typedef RawVec<16>::type RawVec16Any __attribute__((aligned(1)));
__device__ __forceinline__ uint4 nt_load16_any(const unsigned char *p)
{
    const RawVec<16>::type r = __builtin_nontemporal_load(reinterpret_cast<const RawVec16Any *>(p));
    return make_uint4(r.x, r.y, r.z, r.w);
}
__device__ __forceinline__ void nt_store16_any(unsigned char *p, const uint4 &v)
{
    RawVec<16>::type r;
    r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
    __builtin_nontemporal_store(r, reinterpret_cast<RawVec16Any *>(p));
}

// bytes [off, off + 16) of p; those at and past n read as 0 resp. are not written
__device__ inline uint4 load_unit(const unsigned char *p, int64_t off, int64_t n)
{
    const int64_t left = n - off;
    if (left >= 16) return nt_load16_any(p + off);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 16; q++)
        if (q < left) w[q >> 2] |= (uint32_t)p[off + q] << (8 * (q & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ inline void store_unit(unsigned char *p, int64_t off, int64_t n, const uint4 &v)
{
    const int64_t left = n - off;
    if (left >= 16) {
        nt_store16_any(p + off, v);
        return;
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 16; q++)
        if (q < left) p[off + q] = (unsigned char)(w[q >> 2] >> (8 * (q & 3)));
}

}  // namespace pcx
