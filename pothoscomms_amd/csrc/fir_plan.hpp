// fir_plan.hpp -- which plan serves a /comms/fir_filter handle: the one place that states, for (element type, taps, L, M, K, requested
// algorithm), the kernel family a call runs and the algorithm it reports.  Plain C++: no HIP, no allocation; pcx_fir_api.hip builds
// the tables of the plan named here and launches it, tests/fir_plan_main.cpp runs the same functions on the CPU.
//
// fir_plan() is run when the handle's settings change; fir_resolve() is all a call does.
//
// The frequency-domain plans, by element type (K = ceil(ntaps / L); at most one applies to a configuration):
//   complex_float32 / float32, M = L = 1         K <= 2049: CF32_OLS4096 / F32_OLS4096;  2049 < K <= 8193: CF32_UPOLS / F32_UPOLS
//   complex_float32 / float32, L = 1, 1 < M <= 65535, K <= 8193, complex: K > 2049, real: K >= 2               UPOLS_DECIM
//   complex_float32 / float32, 1 < L <= 64, M <= 65535, 2049 < K <= 8193                                       UPOLS_ROWS
//   float32, 1 < L <= 64, M <= 65535, 2 <= K <= 2049                                                           F32_OLS4096_ROWS
//   complex_float32, L > 1 or M > 1, L <= 64, M < 2^17, K <= 2049 (the polyphase family):
//       L = 1, M = 2 or 4 | M, M / fold <= 65535                                                                CF32_DECIM
//       M = 1, L in 2 / 4 / 8 / 16, ntaps <= 2049, K - 1 rounded up to 16 / L within 2048 / L                   CF32_INTERP
//       M = 1 otherwise                                                                                         CF32_OLS4096_ROWS
//       everything else                                                                                         CF32_POLY
//   complex / real float64, int16, int8, M <= 65535, K >= 2, integers while the Q-format taps keep the double pipeline exact:
//       L = 1, K <= 4097: CF64_OLS / REAL64_OLS;   1 < L <= 64, K <= 2049: CF64_OLS_ROWS / REAL64_OLS_ROWS
//   int32, int64: none.
// AUTO takes the plan from auto_min_taps on; a forced PCX_FIR_OLS_FFT takes it at any K and is refused where there is none.
#pragma once
#include <cstddef>

#include "pcx.h"

namespace pcx {

constexpr size_t kOlsMaxTaps = 8193;
// complex_float64 (fir_ols_f64.hip): 4096-sample blocks to K = 2049, 8192 to K = 4097; PCX_OLS64_N forces a plan (A/B)
constexpr size_t kOls64MaxTaps = 4097;
// below this many taps the sliding-window kernel is the faster complex_float64 form (tools/sweep_fir_f64.py: 128 vs 112 Gsamples/s at K = 2)
constexpr size_t kOls64MinTaps = 4;

// Everything the choice depends on.  The diagnostic overrides are plain values: the caller reads the environment, never this header.
struct FirPlanIn {
    int scalar = PCX_F32, cplx = 1, ctaps = 1;
    size_t ntaps = 1, L = 1, M = 1;
    bool taps16 = false;     // complex_int16 / complex_int8, complex Q taps within +-32767 (the packed dot-product kernel's range)
    bool exact = true;       // int16 / int8: ||h_q||^2 < 2^44 for every polyphase row of L (L = 1: the whole tap vector), so that the
                             // rounded sums of the double pipeline are the integer convolution bit for bit
    size_t ols_int_min = 0;  // PCX_OLS_INT_MIN, 0 = the measured default
    size_t ols_real_min = 0; // PCX_OLS_REAL_MIN, 0 = the measured default
    int ols64_n = 0;         // PCX_OLS64_N: 8192 forces the long block of the complex double plans
    bool decim_fullrate = false;   // PCX_FIR_DECIM_FULLRATE: keeps the full-rate evaluation of the polyphase kernel (no folded / replicated spectrum)
    bool poly_strided = false;     // PCX_FIR_POLY_STRIDED: keeps the polyphase kernel's stride-L stores for M = 1 interpolators
    bool slide = true;       // PCX_FIR_SLIDE=0 keeps the one-output-per-lane kernel for M = L = 1 too
    bool dot2 = true;        // PCX_FIR_DOT2=0 keeps complex_int16 on the 24-bit multiply path
    // (taps24 is not here: it picks an instantiation inside launch_fir_slide, not a plan)
};

struct FirPlan {
    size_t K = 1;
    int ols_plan = PCX_FIR_PLAN_NONE;   // the one frequency-domain plan that can serve the configuration
    size_t auto_min_taps = 0;           // AUTO takes ols_plan from this K on
    int td_algo = PCX_FIR_DIRECT;       // the time-domain algorithm AUTO takes otherwise
    int direct_plan = PCX_FIR_PLAN_GENERIC, exact_plan = PCX_FIR_PLAN_GENERIC;   // the time-domain plan under DIRECT / under EXACT
    int td_plan() const { return td_algo == PCX_FIR_DIRECT ? direct_plan : exact_plan; }
    // table parameters of ols_plan
    int parts = 0;       // CF32_ / F32_UPOLS, UPOLS_DECIM, UPOLS_ROWS: tap partitions of 2048 (fir_ols_part.hip)
    int log2n = 0;       // the double-precision plans: log2 of the block (12, 13)
    size_t fold = 1;     // CF32_DECIM: the factor of M folded into the spectrum
};

struct FirChoice {
    int algo, plan;
    bool refused;        // a forced PCX_FIR_OLS_FFT that no plan serves
};

// Tap partitions of the overlap-save plan for K taps (complex_float32, M = L = 1): 0 = the dedicated 4096-sample kernel alone
// (fir_ols.hip, K <= 2049); P = 2 .. 4 = the same blocks with the taps in P partitions of 2048 (fir_ols_part.hip, 2049 < K <= 8193).
// (Until round 6 longer filters took 8192- / 16384-sample blocks on radix-16 family passes -- 143 / 88 Gsamples/s at 4097 / 8193
// taps against 206 / 167 now, profiles/r06/ab_upols.txt; blocks SHORTER than 4096 never paid either: 0.2413 ms at 2048, 0.2723 at
// 1024 against 0.2246 at 255 taps, round 2.)
inline int fir_ols_partitions(size_t K) { return K <= 2049 ? 0 : (int)((K - 1 + 2047) / 2048); }

// even M = M1 * M2: M1 = 16 / 8 / 4 / 2 folded into the spectrum, the cofactor kept one in M2 on the store (the launcher's own
// fir_decim_fold_factor, fir_ols_decim.hip, states the same line)
inline size_t fir_fold_factor(size_t M) { return M % 16 == 0 ? 16 : M % 8 == 0 ? 8 : M % 4 == 0 ? 4 : M % 2 == 0 ? 2 : 1; }

// complex_int16 / complex_int8 on the double pipeline (bit-exact): 166-170 / 128-131 Gsamples/s whatever the tap count, so it
// takes over where the packed dot-product kernel falls below that (tools/sweep_fir_int.py: 164 Gsamples/s at 63 taps, 91 at
// 127, 48 at 255, 12 at 1023); PCX_OLS_INT_MIN overrides (A/B)
inline size_t fir_ols_int_min_taps(const FirPlanIn &c) { return c.ols_int_min ? c.ols_int_min : c.scalar == PCX_I16 ? 64 : 96; }

// REAL float64 / int16 / int8 streams on the double pipeline, two real blocks per transform: 234 / 290 / 296 Gsamples/s
// whatever the tap count; the sliding-window kernel is faster below about 24 / 48 / 48 taps (tools/sweep_fir_int.py real:
// float64 278 vs 228 at 16 taps, 202 vs 234 at 32; int16 356 vs 280 at 32, 230 vs 286 at 63); PCX_OLS_REAL_MIN overrides (A/B)
inline size_t fir_ols_real64_min_taps(const FirPlanIn &c) { return c.ols_real_min ? c.ols_real_min : c.scalar == PCX_F64 ? 24 : 48; }

namespace detail {

// complex_float32 / float32.  Measured sweep (tools/sweep_fir.py, 16 Mi samples): the frequency-domain kernel runs at 285-325
// Gsamples/s for every K <= 1023 (197 at K = 2049) while the time-domain tile peaks at 240-256 and falls as 1/K beyond K ~ 48 -- so
// it is the choice whenever it applies.  K == 1 (the block's default unit tap) stays in the time domain where M = L = 1: a
// pass-through filter must return its input bit for bit, as the reference does.
inline void ols_plan_f32(const FirPlanIn &c, FirPlan &p)
{
    const size_t K = p.K;
    auto take = [&](int plan, size_t auto_min, int parts = 0) { p.ols_plan = plan; p.auto_min_taps = auto_min; p.parts = parts; };
    if (c.L == 1 && c.M == 1) {
        // complex: fir_ols.hip, beyond 2049 taps the partitioned kernel; real: two real blocks per complex transform (fir_ols.hip),
        // beyond 2049 taps the two halves of the call side by side through the partitioned kernel (fir_ols_part.hip)
        if (K > kOlsMaxTaps) return;
        const int parts = fir_ols_partitions(K);
        if (c.cplx) take(parts ? PCX_FIR_PLAN_CF32_UPOLS : PCX_FIR_PLAN_CF32_OLS4096, 2, parts);
        else take(parts ? PCX_FIR_PLAN_F32_UPOLS : PCX_FIR_PLAN_F32_OLS4096, 2, parts);
        return;
    }
    if (c.L > 64) return;
    if (K > 2049 || !c.cplx) {
        if (c.M > 65535 || K > kOlsMaxTaps) return;
        // long DECIMATING filters: the partitioned kernel at the full rate, one output in M stored (fir_ols_part.hip) -- the
        // time-domain tile they fell to runs at 1-2 Gsamples/s of input at these tap counts.  REAL float32 decimators of any length
        // take it as well (one partition up to 2049 taps): 300 against the 155 Gsamples/s of the double-precision pipeline they
        // shared with the integer types
        if (c.L == 1 && K >= 2) take(PCX_FIR_PLAN_UPOLS_DECIM, 16, fir_ols_partitions(K) ? fir_ols_partitions(K) : 1);
        // INTERPOLATING filters whose polyphase rows are longer than 2049 taps: every row through the partitioned kernel at the
        // input rate into a workspace row, then the interleaving pass (which also keeps one position in M)
        else if (c.L > 1 && K > 2049) take(PCX_FIR_PLAN_UPOLS_ROWS, 1, fir_ols_partitions(K));
        // interpolating REAL float32 filters: every polyphase row through the real float kernel (fir_ols.hip) into a workspace
        // row, then the interleaving pass
        else if (c.L > 1 && K >= 2) take(PCX_FIR_PLAN_F32_OLS4096_ROWS, 16);
        return;
    }
    // complex_float32, K <= 2049, L > 1 or M > 1: one spectrum per polyphase row, unless a cheaper form of the same filter applies
    if (c.M >= ((size_t)1 << 17)) return;
    const size_t fold = fir_fold_factor(c.M);
    // decimating: one forward transform, the spectrum folded, a 4096/fold-point inverse (fir_ols_decim.hip).  Folding pays from
    // 4-fold on (and for M = 2 itself); 2-fold plus a cofactor measured slower than the full-rate kernel (M = 10: 244 vs 281,
    // M = 50: 251 vs 284 Gsamples/s in; M = 160 = 16 * 10: 373 vs 287)
    if (c.L == 1 && (c.M == 2 || fold >= 4) && c.M / fold <= 65535 && !c.decim_fullrate) {
        take(PCX_FIR_PLAN_CF32_DECIM, 1);
        p.fold = fold;
        return;
    }
    // interpolating: a 4096/L-point forward transform, its spectrum replicated against H of the WHOLE tap vector, the ordinary
    // 4096-point inverse writing the interleaved output stream (fir_ols_decim.hip)
    if (c.M == 1 && (c.L == 2 || c.L == 4 || c.L == 8 || c.L == 16) && !c.decim_fullrate) {
        const size_t A = 16 / c.L, kov_in = (K - 1 + A - 1) / A * A;
        if (kov_in <= 4096 / c.L / 2 && c.ntaps <= 2049) { take(PCX_FIR_PLAN_CF32_INTERP, 1); return; }
    }
    // interpolation by other factors: each polyphase row through the undecimated kernel into a contiguous workspace row, then one
    // interleaving pass; rational resampling and odd decimation: the polyphase kernel's strided stores
    take(c.M == 1 && !c.poly_strided ? PCX_FIR_PLAN_CF32_OLS4096_ROWS : PCX_FIR_PLAN_CF32_POLY, 1);
}

// float64 / int16 / int8, complex or real, on the double-precision pipeline (fir_ols_f64.hip): M > 1 stores one output in M, L > 1
// runs every polyphase row into a workspace row and interleaves.  Decimating complex filters: the full-rate pipeline runs at
// 130-170 Gsamples/s of input whatever K; the one-output-per-lane kernel it replaces measured 45-129 (int16) / 27-31 (float64) at
// 63 taps and 12-33 / 6-8 at 255 (tools/decim_int_probe.py)
inline void ols_plan_f64(const FirPlanIn &c, FirPlan &p)
{
    const size_t K = p.K;
    const bool integer = c.scalar != PCX_F64;
    if (c.M > 65535 || K < 2 || (integer && !c.exact)) return;
    if (c.L == 1 && K <= kOls64MaxTaps) {
        p.ols_plan = c.cplx ? PCX_FIR_PLAN_CF64_OLS : PCX_FIR_PLAN_REAL64_OLS;
        p.log2n = K <= 2049 ? 12 : 13;
        if (c.cplx && c.ols64_n == 8192) p.log2n = 13;     // (the override was never wired to the real plan)
        if (c.cplx) p.auto_min_taps = c.M > 1 ? (integer ? 32 : 16) : integer ? fir_ols_int_min_taps(c) : kOls64MinTaps;
        else p.auto_min_taps = c.M > 1 ? 16 : fir_ols_real64_min_taps(c);
    } else if (c.L > 1 && c.L <= 64 && K <= 2049) {
        p.ols_plan = c.cplx ? PCX_FIR_PLAN_CF64_OLS_ROWS : PCX_FIR_PLAN_REAL64_OLS_ROWS;
        p.log2n = 12;
        p.auto_min_taps = 16;
    }
}

}  // namespace detail

inline FirPlan fir_plan(const FirPlanIn &c)
{
    FirPlan p;
    p.K = c.ntaps / c.L + (c.ntaps % c.L == 0 ? 0 : 1);     // FIRFilter::updateInternals, FIRFilter.cpp:327-354
    if (c.scalar == PCX_F32) detail::ols_plan_f32(c, p);
    else if (c.scalar == PCX_F64 || c.scalar == PCX_I16 || c.scalar == PCX_I8) detail::ols_plan_f64(c, p);

    // the time-domain kernels: the sliding-window ones for M = L = 1, one output per lane otherwise
    const bool unit = c.L == 1 && c.M == 1, fast = c.scalar == PCX_F32 && c.cplx && unit;
    const int sliding = c.slide && c.dot2 && c.taps16 && unit && p.K <= 12000 ? PCX_FIR_PLAN_DOT2
                      : c.slide && unit ? PCX_FIR_PLAN_SLIDE : PCX_FIR_PLAN_GENERIC;
    // complex_float32, M = L = 1 under DIRECT: the LDS-tiled kernel while its tile (2048 outputs + taps) fits
    const size_t Kp = (p.K + 7) / 8 * 8;
    p.direct_plan = fast && (2048 + Kp + 8) * 9 / 8 * 8 + 64 <= 64 * 1024 ? PCX_FIR_PLAN_CF32_DIRECT_TILE : sliding;
    p.exact_plan = sliding;
    // longer than every frequency-domain plan (K > 8193): the sliding-window kernel in the reference's own operation order -- 8k-term
    // float sums accumulate enough rounding that a reordered sum would sit on the 1e-5 bar
    if (fast) p.td_algo = p.K > kOlsMaxTaps ? PCX_FIR_EXACT : PCX_FIR_DIRECT;
    else p.td_algo = c.scalar == PCX_F32 || c.scalar == PCX_F64 ? PCX_FIR_DIRECT : PCX_FIR_EXACT;
    return p;
}

// the algorithm and plan of one call under the handle's requested algorithm
inline FirChoice fir_resolve(const FirPlan &p, int requested)
{
    const bool have = p.ols_plan != PCX_FIR_PLAN_NONE;
    switch (requested) {
    case PCX_FIR_OLS_FFT: return {PCX_FIR_OLS_FFT, p.ols_plan, !have};
    case PCX_FIR_DIRECT: return {PCX_FIR_DIRECT, p.direct_plan, false};
    case PCX_FIR_EXACT: return {PCX_FIR_EXACT, p.exact_plan, false};
    }
    if (have && p.K >= p.auto_min_taps) return {PCX_FIR_OLS_FFT, p.ols_plan, false};
    return {p.td_algo, p.td_plan(), false};
}

}  // namespace pcx
