// ols_block.hpp -- the steps that the overlap-save /comms/fir_filter kernels on the 4096-point float32 transform share
// (fir_ols.hip, fir_ols_decim.hip): one copy of each, inlined into every kernel that takes it.  Include after fft4096.hpp.
//
// What is here are the steps that live in registers: the spectrum multiply and the lane's part of the resampling kernels'
// short transform.  Every kernel that calls one compiles to the instructions it had with the step written out.  The steps
// around a memory access -- the window fetch, the 256-point sub-transforms through LDS, the row stores -- do NOT: taken out of
// a kernel into a function they come back with another register assignment and another instruction order (what their unrolled
// loops hold that does not change from block to block -- row tests, row offsets, descriptor bases -- is hoisted to another place
// in the kernel's prologue), in kernels that are a few registers from spilling.  Those stay written out where they are -- but for the
// full-block window fetch and the policy select of a row store of the two complex_float32 kernels of fir_ols.hip (below), which
// compile to the parent's instructions (profiles/r08/resource_usage.txt).
// The `asm volatile("" : "+v"(..))` / "+s" pins that keep a loop-invariant load inside a kernel's block loop are decisions of
// that kernel and stay at its call site: these functions take the pinned pointer.
#pragma once
#include "fft4096.hpp"

namespace pcx {
namespace fft4k {

// ---- which stream rows take the default cache policy ----
// A block's window is sixteen 2 KiB rows, row r = samples 256 r .. 256 r + 255, and so is what it stores.  A row mask has bit r set for a
// row accessed on the DEFAULT cache policy; the other rows are non-temporal.  Consecutive blocks overlap by Kov samples: the
// ceil(Kov / 256) rows at either end of a window are read by a neighbouring block as well and MUST be in a load mask (their second
// reader hits in L2: that holds HBM traffic at 1.03 x algorithmic).  What a mask holds beyond them is tuning
// (tools/floor_lab.hip `rows`).
constexpr unsigned kRowsAll = 0xFFFFu, kRowsNone = 0u;
constexpr unsigned rows_ends(int n) { return ((1u << n) - 1u) | (((1u << n) - 1u) << (16 - n)); }     // n rows at either end, n = 1 .. 8
// the largest n with rows_ends(n) inside the mask: a launcher may give the mask to overlaps Kov <= 256 n, and to no larger one
constexpr int rows_shared_kept(unsigned mask)
{
    int n = 0;
    while (n < 8 && (rows_ends(n + 1) & ~mask) == 0) n++;
    return n;
}

// ---- the window fetch of a full block (the fast path: every row inside the buffer) ----
// dst[r] = row r of the window behind the descriptor, lane j on column j: sixteen unconditional raw_buffer_load_b64, the policy of each a
// compile-time bit of DEFAULT_ROWS (the select below folds per row once the loop is unrolled: no branch reaches the ISA).
// PAIRED = false: the row's displacement 2048 r in the scalar offset (fir_cf32_ols4096_kernel); true: the odd rows' 2048 in the
// instruction's 12-bit offset field, so that eight scalar offsets serve sixteen rows (fmchain_cf32_ols4096_kernel).
template <unsigned DEFAULT_ROWS, bool PAIRED>
__device__ __forceinline__ void load_window_rows(cf (&dst)[16], __amdgpu_buffer_rsrc_t rs, int j)
{
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int voff = PAIRED ? j * 8 + 2048 * (r & 1) : j * 8, soff = PAIRED ? 4096 * (r >> 1) : 2048 * r;
        const u32x2 t = ((DEFAULT_ROWS >> r) & 1u) ? __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0)
                                                   : __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 2);
        dst[r] = cf{__uint_as_float(t.x), __uint_as_float(t.y)};
    }
}
// one row of the sixteen a block stores: the default policy if DEFAULT_ROWS has bit `row`, else OTHER_AUX (2 = non-temporal)
// (`row` is a constant wherever the caller's row loop is unrolled: the select folds, as above)
template <unsigned DEFAULT_ROWS, int OTHER_AUX>
__device__ __forceinline__ void store_row_cf(__amdgpu_buffer_rsrc_t ws, unsigned voff, cf a, int row)
{
    if ((DEFAULT_ROWS >> row) & 1u) store_cf<0>(ws, voff, a);
    else store_cf<OTHER_AUX>(ws, voff, a);
}

// ---- spectrum times H ----
// v[q] = X[.. + 256 bin_of(q)] as the forward passes leave it; u[r] = conj(X * H) in natural register order r for the first
// pass of the inverse.  The inverse transform runs on the FORWARD passes: IFFT(z) = conj(FFT(conj(z))), so one set of twiddles
// serves both directions; the final conj rides on the last additions of the inverse's third pass.
// H: the lane's sixteen bins held in registers
__device__ __forceinline__ void spectrum_times_h(cf (&u)[16], const cf (&v)[16], const cf (&H)[16])
{
#pragma unroll
    for (int q = 0; q < 16; q += 2) {
        const int k0 = bin_of(q), k1 = bin_of(q + 1);
        u[k0] = v[q];
        u[k1] = v[q + 1];
        cmul2_conj(u[k0], u[k1], H[k0], H[k1]);
    }
}
// The same multiply folded into the inner layer of the inverse's first sixteen-point transform (fft4096.hpp, folded butterflies): every
// input of that layer's DFT4s is a product conj(X H), so each pair of products and its butterfly take five packed instructions instead
// of six.  On exit u is where fft16_inner leaves it: what dit_back<.., true> takes.  Register k of the natural order is v[bin_of(k)].
__device__ __forceinline__ void spectrum_times_h_inner(cf (&u)[16], const cf (&v)[16], const cf (&H)[16])
{
#pragma unroll
    for (int n2 = 0; n2 < 4; n2++) {
        cf x0 = v[4 * n2], x1 = v[4 * n2 + 1], x2 = v[4 * n2 + 2], x3 = v[4 * n2 + 3];      // v[bin_of(4 n1 + n2)]
        cf m0, m1;
        // m0 = conj(h0 x0), t0 = m0 + conj(h2 x2) -> x2, t1 = 2 m0 - t0 -> x0; m1 = conj(h1 x1), t2 = m1 + conj(h3 x3) -> x3, d -> x1;
        // then the DFT4's four additions in the same block (a compiler-made addition behind it would take a wait state)
        asm("v_pk_mul_f32 %4, %0, %6" PCX_FOLD_IMC0 "\n\t"
            "v_pk_mul_f32 %5, %1, %7" PCX_FOLD_IMC0 "\n\t"
            "v_pk_fma_f32 %4, %0, %6, %4" PCX_FOLD_REC "\n\t"
            "v_pk_fma_f32 %5, %1, %7, %5" PCX_FOLD_REC "\n\t"
            "v_pk_fma_f32 %0, %2, %8, %4" PCX_FOLD_IMC "\n\t"
            "v_pk_fma_f32 %1, %3, %9, %5" PCX_FOLD_IMC "\n\t"
            "v_pk_fma_f32 %2, %2, %8, %0" PCX_FOLD_REC "\n\t"
            "v_pk_fma_f32 %3, %3, %9, %1" PCX_FOLD_REC "\n\t"
            "v_pk_fma_f32 %0, %4, 2.0, %2" PCX_FOLD_2AMP "\n\t"
            "v_pk_fma_f32 %1, %5, 2.0, %3" PCX_FOLD_2AMP "\n\t"
            "v_pk_add_f32 %4, %2, %3\n\t"                                                     // t0 + t2
            "v_pk_add_f32 %2, %2, %3 neg_lo:[0,1] neg_hi:[0,1]\n\t"                           // t0 - t2
            "v_pk_add_f32 %5, %0, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]\n\t"           // t1 + (-i) d
            "v_pk_add_f32 %3, %0, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]"               // t1 - (-i) d
            : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "=&v"(m0), "=&v"(m1)
            : "v"(H[n2]), "v"(H[4 + n2]), "v"(H[8 + n2]), "v"(H[12 + n2]));
        u[n2] = m0;
        u[4 + n2] = m1;
        u[8 + n2] = x2;
        u[12 + n2] = x3;
    }
}
// Hb: the lane's bin 0 in the spectrum, the others 256 elements apart -- re-read from L2 in every block
__device__ __forceinline__ void spectrum_times_h_l2(cf (&u)[16], const cf (&v)[16], const cf *Hb)
{
#pragma unroll
    for (int q = 0; q < 16; q += 2) {
        const int k0 = bin_of(q), k1 = bin_of(q + 1);
        u[k0] = v[q];
        u[k1] = v[q + 1];
        cmul2_conj(u[k0], u[k1], Hb[256 * k0], Hb[256 * k1]);
    }
}
// the interpolators: zero-stuffing by 16/P replicates the 256 P-point spectrum g, u[r] = conj(g[r mod P] * H[r])
template <int P>
__device__ __forceinline__ void replicated_times_h(cf (&u)[16], const cf (&g)[P], const cf (&H)[16])
{
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        u[r] = g[r & (P - 1)];
        u[r + 1] = g[(r + 1) & (P - 1)];
        cmul2_conj(u[r], u[r + 1], H[r], H[r + 1]);
    }
}
template <int P>
__device__ __forceinline__ void replicated_times_h_l2(cf (&u)[16], const cf (&g)[P], const cf *Hb)
{
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        u[r] = g[r & (P - 1)];
        u[r + 1] = g[(r + 1) & (P - 1)];
        cmul2_conj(u[r], u[r + 1], Hb[256 * r], Hb[256 * (r + 1)]);
    }
}

// ---- the lane's part of the 256 P-point transform of the resampling kernels ----
// W_{256 P}^js: the lane constant of the radix-P stage, js = spec_lane(j): the lane's bins are js + 256 r.  Its powers
// 2 .. P-1 are rebuilt by multiplication in every block: 6 packed multiplies against 12 more registers.
template <int P>
__device__ __forceinline__ cf radix_stage_twiddle(int js)
{
    float sn, cs;
    sincospif(-2.0f * (float)js / (float)(256 * P), &sn, &cs);
    return cf{cs, sn};
}
// the decimators: radix-P decimation-in-frequency stage over the lane's P folded values, then the lane twiddle td1^k1 on value k1
template <int P>
__device__ __forceinline__ void radix_stage_dif(cf (&z)[P], cf td1)
{
    if constexpr (P == 8) fft8(z[0], z[1], z[2], z[3], z[4], z[5], z[6], z[7]);
    else if constexpr (P == 4) fft4(z[0], z[1], z[2], z[3]);
    else if constexpr (P == 2) { const cf a = z[0], c = z[1]; z[0] = a + c; z[1] = a - c; }
    cf t = td1;
#pragma unroll
    for (int k1 = 1; k1 < P; k1++) {
        z[k1] = cmul1(z[k1], t);
        if (k1 + 1 < P) t = cmul1(t, td1);
    }
}

}  // namespace fft4k
}  // namespace pcx
