// repack_core.hpp -- the word arithmetic of the four repacking blocks (repack.hip): eight symbols at a time in one
// 64-bit word, every shift and mask a constant of the instantiation.  Plain C++ on purpose: a host compiler runs the same functions
// (tests/test_repack_cpu.py holds them against the recorded outputs of the reference's loops for every kind, width and order).
//
// A GROUP is eight symbols of W bits and the W bytes that hold them.  In both bit orders the W bytes are read as one number G of 8 W
// bits in which field k occupies bits [W k, W k + W):
//   LSBit   G is the little-endian reading of the bytes, field k is symbol k
//   MSBit   G is the big-endian reading of the bytes,    field k is symbol 7 - k
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PCX_HD __host__ __device__ __forceinline__
#else
#define PCX_HD inline
#endif

namespace pcx {
namespace repack {

PCX_HD uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
PCX_HD uint64_t bswap64(uint64_t v) { return __builtin_bswap64(v); }

// ---------------------------------------------------------------- bytes -> symbols (and the second half of bits -> symbols)
// four fields of W bits in the low 4 W bits of h, each into a byte of its own: two doubling steps, every field moved at once
template <int W>
PCX_HD uint32_t spread4(uint32_t h)
{
    constexpr uint32_t m2 = (1u << (2 * W)) - 1, m1 = (1u << W) - 1, M1 = m1 | (m1 << 16);
    h = (h & m2) | (((h >> (2 * W)) & m2) << 16);
    return (h & M1) | ((h & (M1 << W)) << (8 - W));
}
// v: the W bytes of a group, little-endian (the first byte of the stream lowest); returns the eight symbols, symbol j in byte j
template <int W, bool MSB>
PCX_HD uint64_t extract8(uint64_t v)
{
    if constexpr (W == 8) {
        return v;
    } else {
        constexpr uint32_t m4 = (uint32_t)((1ull << (4 * W)) - 1);
        const uint64_t g = MSB ? bswap64(v) >> (64 - 8 * W) : v;
        const uint32_t lo = spread4<W>((uint32_t)g & m4), hi = spread4<W>((uint32_t)(g >> (4 * W)) & m4);      // fields 0..3, 4..7
        if constexpr (MSB) return (uint64_t)bswap32(hi) | ((uint64_t)bswap32(lo) << 32);                        // byte j = field 7 - j
        else return (uint64_t)lo | ((uint64_t)hi << 32);
    }
}

// ---------------------------------------------------------------- symbols -> bytes (and the first half of symbols -> bits)
// THE CLIPPED OR.  The reference ORs shifted symbols that it never masks and truncates each result to a byte
// (SymbolHelpers.hpp:77-228).  What that computes, for every width and both orders: the whole 8-bit value of the symbol of field k
// is placed with its bit 0 on bit W k of G, and is cut off at the upper edge of the last byte its FIELD touches:
//     G = OR over k of (value_k << W k) restricted to bits [W k, min(W k + 8, 8 (floor((W k + W - 1) / 8) + 1)))
// Bits of a value above its width so land on the fields above it, never beyond the byte in which its own field ends.
template <int W, int K>
constexpr uint64_t field_mask()
{
    constexpr int p = W * K, top = 8 * ((p + W - 1) / 8 + 1), end = p + 8 < top ? p + 8 : top;
    return (end >= 64 ? ~0ull : (1ull << end) - 1) & ~((1ull << p) - 1);
}
template <int W, int K>
PCX_HD uint64_t field_term(uint64_t x) { return (x >> ((8 - W) * K)) & field_mask<W, K>(); }      // x: the value of field k in byte k
// s: eight symbols, symbol j in byte j; returns the W bytes of the group, little-endian.  MASKED: only the low W bits of a symbol count
template <int W, bool MSB, bool MASKED>
PCX_HD uint64_t pack8(uint64_t s)
{
    if constexpr (W == 8) {
        return s;
    } else {
        if constexpr (MASKED) s &= 0x0101010101010101ull * ((1u << W) - 1);
        const uint64_t x = MSB ? bswap64(s) : s;
        const uint64_t g = field_term<W, 0>(x) | field_term<W, 1>(x) | field_term<W, 2>(x) | field_term<W, 3>(x) | field_term<W, 4>(x) |
                           field_term<W, 5>(x) | field_term<W, 6>(x) | field_term<W, 7>(x);
        return MSB ? bswap64(g << (64 - 8 * W)) : g;
    }
}

// ---------------------------------------------------------------- a lane's W words: four groups of W bytes
template <int OFF, int LEN, int NW>
PCX_HD uint64_t get_bytes(const uint32_t (&w)[NW])
{
    constexpr int i0 = OFF / 4, sh = 8 * (OFF % 4);
    uint64_t v = w[i0];
    if constexpr (i0 + 1 < NW) v |= (uint64_t)w[i0 + 1] << 32;
    v >>= sh;
    if constexpr (sh != 0 && i0 + 2 < NW && sh + 8 * LEN > 64) v |= (uint64_t)w[i0 + 2] << (64 - sh);
    if constexpr (LEN < 8) v &= (1ull << (8 * LEN)) - 1;
    return v;
}
// g < 2^(8 LEN) is ORed into bytes [OFF, OFF + LEN)
template <int OFF, int LEN, int NW>
PCX_HD void put_bytes(uint32_t (&w)[NW], uint64_t g)
{
    constexpr int i0 = OFF / 4, sh = 8 * (OFF % 4);
    const uint64_t s = g << sh;
    w[i0] |= (uint32_t)s;
    if constexpr (i0 + 1 < NW && sh + 8 * LEN > 32) w[i0 + 1] |= (uint32_t)(s >> 32);
    if constexpr (sh != 0 && i0 + 2 < NW && sh + 8 * LEN > 64) w[i0 + 2] |= (uint32_t)(g >> (64 - sh));
}
// 32 symbols (8 words, symbol j in byte j) <-> their 4 W bytes (W words)
template <int W, bool MSB>
PCX_HD void extract32(const uint32_t (&p)[W], uint32_t (&s)[8])
{
    const uint64_t a = extract8<W, MSB>(get_bytes<0, W, W>(p)), b = extract8<W, MSB>(get_bytes<W, W, W>(p));
    const uint64_t c = extract8<W, MSB>(get_bytes<2 * W, W, W>(p)), d = extract8<W, MSB>(get_bytes<3 * W, W, W>(p));
    s[0] = (uint32_t)a; s[1] = (uint32_t)(a >> 32); s[2] = (uint32_t)b; s[3] = (uint32_t)(b >> 32);
    s[4] = (uint32_t)c; s[5] = (uint32_t)(c >> 32); s[6] = (uint32_t)d; s[7] = (uint32_t)(d >> 32);
}
template <int W, bool MSB, bool MASKED>
PCX_HD void pack32(const uint32_t (&s)[8], uint32_t (&p)[W])
{
#pragma unroll
    for (int i = 0; i < W; i++) p[i] = 0;
    put_bytes<0, W, W>(p, pack8<W, MSB, MASKED>((uint64_t)s[0] | ((uint64_t)s[1] << 32)));
    put_bytes<W, W, W>(p, pack8<W, MSB, MASKED>((uint64_t)s[2] | ((uint64_t)s[3] << 32)));
    put_bytes<2 * W, W, W>(p, pack8<W, MSB, MASKED>((uint64_t)s[4] | ((uint64_t)s[5] << 32)));
    put_bytes<3 * W, W, W>(p, pack8<W, MSB, MASKED>((uint64_t)s[6] | ((uint64_t)s[7] << 32)));
}

// ---------------------------------------------------------------- bit per byte <-> bit per bit
// a, b: bytes 0..7 and 8..15 of sixteen one-bit-per-byte inputs; returns their sixteen flags (byte != 0) as two bytes of the bit stream,
// the first input on the lowest (LSBit) or the highest (MSBit) bit of the first byte.  The test runs on eight bytes at once: adding
// 0x7f to the low seven bits of a byte carries into bit 7 exactly when one of them is set.  Four flags then meet in one nibble by one
// multiplication: the products 2^(8 i) 2^(7 j + 7) (LSBit) and 2^(8 i) 2^(9 j + 4) (MSBit) have distinct exponents, so nothing carries.
PCX_HD uint64_t nonzero_flags(uint64_t v)
{
    constexpr uint64_t k7f = 0x7f7f7f7f7f7f7f7full;
    return ((((v & k7f) + k7f) | v) >> 7) & 0x0101010101010101ull;
}
template <bool MSB>
PCX_HD uint32_t gather4(uint32_t flags) { return (flags * (MSB ? 0x80402010u : 0x10204080u)) >> 28; }
template <bool MSB>
PCX_HD uint32_t gather16(uint64_t a, uint64_t b)
{
    const uint64_t fa = nonzero_flags(a), fb = nonzero_flags(b);
    const uint32_t n0 = gather4<MSB>((uint32_t)fa), n1 = gather4<MSB>((uint32_t)(fa >> 32));
    const uint32_t n2 = gather4<MSB>((uint32_t)fb), n3 = gather4<MSB>((uint32_t)(fb >> 32));
    if constexpr (MSB) return (n0 << 4) | n1 | (n2 << 12) | (n3 << 8);
    else return n0 | (n1 << 4) | (n2 << 8) | (n3 << 12);
}
// a nibble of the bit stream into four bytes of 0 / 1, its first bit (bit 0 of the nibble: LSBit, bit 3: MSBit) into byte 0
template <bool MSB>
PCX_HD uint32_t spread_nibble(uint32_t n)
{
    if constexpr (MSB) return ((n * 0x08040201u) >> 3) & 0x01010101u;
    else return (n * 0x00204081u) & 0x01010101u;
}
// two bytes of the bit stream (the first lowest) into sixteen bytes
template <bool MSB>
PCX_HD void spread16(uint32_t v, uint32_t (&o)[4])
{
    if constexpr (MSB) {
        o[0] = spread_nibble<true>((v >> 4) & 15u); o[1] = spread_nibble<true>(v & 15u);
        o[2] = spread_nibble<true>((v >> 12) & 15u); o[3] = spread_nibble<true>((v >> 8) & 15u);
    } else {
        o[0] = spread_nibble<false>(v & 15u); o[1] = spread_nibble<false>((v >> 4) & 15u);
        o[2] = spread_nibble<false>((v >> 8) & 15u); o[3] = spread_nibble<false>((v >> 12) & 15u);
    }
}

}  // namespace repack
}  // namespace pcx
