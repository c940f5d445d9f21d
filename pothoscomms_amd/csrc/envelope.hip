// envelope.hip -- /comms/envelope_detector (filter/EnvelopeDetector.cpp:110-148): per output
//   x = |in[i + lookahead]| narrowed to float,  e = (x > e) ? gA*e + oA*x : gR*e + oR*x,  out[i] = e
// with the same bits as the sequential float32 loop.  The branch depends on the state, so there is no scan; the
// recurrence is a contraction instead, and two trajectories started from different states become bit-identical after a while and
// stay so.  One call slice runs as three launches, whatever the data:
//   speculate  one thread per chunk of C samples: a warm-up over the W samples in front of the chunk from state 0 (chunks whose
//              warm-up reaches the slice start begin from the carried state, exactly), then the chunk, outputs written, end state
//              recorded in ends[c]
//   repair     chunk c >= 1 again from ends[c-1], until the new state equals the stored output BIT FOR BIT; the outputs in front of
//              that point are overwritten.  A chunk that never matches is exact itself, but its successor started from a wrong
//              ends[c]: it is marked, and counted
//   resolve    one thread: when something was marked, the marked chunks in order from the true end of their predecessor (a chunk
//              re-run to its end without a match carries the mark on); then the carried state := the last output
// Products and sums are rounded separately (the tree builds with -ffp-contract=off), f32 subnormals are kept (hipcc's default
// mode), and every sample index is 64-bit.
#include "pcx_internal.hpp"

namespace pcx {
namespace {

constexpr int kNT = 256;        // threads per workgroup (speculate, repair)
constexpr int kB = 16;          // samples a thread loads ahead of its recurrence

__device__ inline float env_step(float e, float x, const EnvGains &g)
{
    const float ax = g.oA * x, rx = g.oR * x;      // (independent of the state)
    const float up = g.gA * e + ax, down = g.gR * e + rx;
    return x > e ? up : down;
}

// x86-64 cvttsd2si, what g++ emits for double -> int32 / int64: out of range or NaN gives the minimum of the type
__device__ inline int32_t trunc_i32(double v)
{
    return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN;
}
__device__ inline int64_t trunc_i64(double v)
{
    return (v >= -9223372036854775808.0 && v < 9223372036854775808.0) ? (int64_t)v : INT64_MIN;
}

// libstdc++'s generic __complex_abs for complex<T>, T an integer (the C99 cabs path covers floats only): s = T(max(abs(re),
// abs(im))) with abs in the promoted type (abs(INT_MIN) stays INT_MIN); re /= s, im /= s in T; s * sqrt(re*re + im*im) in double,
// truncated back to T.  Products wrap as the compiled header's do.
template <typename T>
__device__ inline float cplx_int_abs(T re, T im)
{
    if constexpr (sizeof(T) == 8) {
        const int64_t ar = re < 0 ? (int64_t)(0 - (uint64_t)re) : re, ai = im < 0 ? (int64_t)(0 - (uint64_t)im) : im;
        const int64_t s = ar > ai ? ar : ai;
        if (s == 0) return 0.0f;
        const int64_t x = re / s, y = im / s;            // (s >= 1 or INT64_MIN: no quotient overflows)
        const int64_t m2 = (int64_t)((uint64_t)x * (uint64_t)x + (uint64_t)y * (uint64_t)y);
        return (float)trunc_i64((double)s * sqrt((double)m2));
    } else if constexpr (sizeof(T) == 4) {
        const int32_t ar = re < 0 ? (int32_t)(0u - (uint32_t)re) : re, ai = im < 0 ? (int32_t)(0u - (uint32_t)im) : im;
        const int32_t s = ar > ai ? ar : ai;
        if (s == 0) return 0.0f;
        const int32_t x = re / s, y = im / s;
        const int32_t m2 = (int32_t)((uint32_t)x * (uint32_t)x + (uint32_t)y * (uint32_t)y);
        return (float)trunc_i32((double)s * sqrt((double)m2));
    } else {
        const int ar = re < 0 ? -(int)re : (int)re, ai = im < 0 ? -(int)im : (int)im;
        const T s = (T)(ar > ai ? ar : ai);
        if (s == 0) return 0.0f;
        const T x = (T)((int)re / (int)s), y = (T)((int)im / (int)s);
        const int m2 = (int)x * (int)x + (int)y * (int)y;
        return (float)(T)trunc_i32((double)s * sqrt((double)m2));
    }
}

// getAbs<float>(in[i]) of EnvelopeDetector.cpp (functions/FxptHelpers.hpp: float(std::abs(in)))
template <typename T, bool CPLX>
__device__ inline float env_mag(const T *__restrict__ in, int64_t i)
{
    if constexpr (!CPLX) {
        const T v = in[i];
        if constexpr (std::is_floating_point<T>::value) return (float)fabs(v);
        else if constexpr (sizeof(T) < 4) return (float)(v < 0 ? -(int)v : (int)v);        // abs of the promoted int
        else {
            using U = typename std::make_unsigned<T>::type;
            return (float)(v < 0 ? (T)((U)0 - (U)v) : v);                                // abs(INT_MIN) = INT_MIN
        }
    } else {
        const T a = in[2 * i], b = in[2 * i + 1];
        if constexpr (std::is_same<T, float>::value) {
            // hypotf (glibc 2.35): (float)sqrt((double)a*a + (double)b*b) after the inf cases; elementwise.hip's AbsCplxF32
            if (isinf(a) || isinf(b)) return INFINITY;
            const double da = (double)a, db = (double)b;
            return (float)sqrt(da * da + db * db);
        } else if constexpr (std::is_same<T, double>::value) {
            return (float)hypot(a, b);                                                   // elementwise.hip's AbsCplxF64
        } else {
            return cplx_int_abs<T>(a, b);
        }
    }
}

__device__ inline bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }

// the recurrence over [a, b) from e; outputs written when out is given.  Magnitudes are loaded kB ahead of the chain.
template <typename T, bool CPLX>
__device__ inline float env_run(const T *__restrict__ in, float *__restrict__ out, int64_t a, int64_t b, float e, const EnvGains &g)
{
    int64_t i = a;
    for (; i + kB <= b; i += kB) {
        float x[kB];
#pragma unroll
        for (int j = 0; j < kB; j++) x[j] = env_mag<T, CPLX>(in, i + j);
#pragma unroll
        for (int j = 0; j < kB; j++) {
            e = env_step(e, x[j], g);
            if (out) out[i + j] = e;
        }
    }
    for (; i < b; i++) {
        e = env_step(e, env_mag<T, CPLX>(in, i), g);
        if (out) out[i] = e;
    }
    return e;
}

// [a, b) from e against the stored outputs: stops at the first state whose bits equal the stored one (returns true), overwrites
// the outputs in front of it; *rewrote: at least one output changed
template <typename T, bool CPLX>
__device__ inline bool env_mend(const T *__restrict__ in, float *__restrict__ out, int64_t a, int64_t b, float e, const EnvGains &g,
                                bool *rewrote)
{
    int64_t i = a;
    for (; i + kB <= b; i += kB) {
        float x[kB], o[kB];
#pragma unroll
        for (int j = 0; j < kB; j++) { x[j] = env_mag<T, CPLX>(in, i + j); o[j] = out[i + j]; }
#pragma unroll
        for (int j = 0; j < kB; j++) {
            e = env_step(e, x[j], g);
            if (same_bits(e, o[j])) return true;
            out[i + j] = e;
            *rewrote = true;
        }
    }
    for (; i < b; i++) {
        e = env_step(e, env_mag<T, CPLX>(in, i), g);
        if (same_bits(e, out[i])) return true;
        out[i] = e;
        *rewrote = true;
    }
    return false;
}

enum { kSuspect = 0, kChunks = 1, kRepaired = 2, kResolved = 3 };

template <typename T, bool CPLX>
__global__ __launch_bounds__(kNT) void env_spec_kernel(const T *__restrict__ in, float *__restrict__ out, int64_t n, int64_t C,
                                                        int64_t W, int64_t nch, const float *__restrict__ state,
                                                        float *__restrict__ ends, unsigned long long *__restrict__ cnt, int first,
                                                        EnvGains g)
{
    const int64_t c = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (c == 0) {
        // (the counters are read by later launches only)
        cnt[kSuspect] = 0;
        cnt[kChunks] = (first ? 0 : cnt[kChunks]) + (unsigned long long)nch;
        if (first) cnt[kRepaired] = cnt[kResolved] = 0;
    }
    if (c >= nch) return;
    const int64_t s0 = c * C, s1 = s0 + C < n ? s0 + C : n;
    const int64_t w0 = s0 > W ? s0 - W : 0;
    float e = w0 == 0 ? *state : 0.0f;
    e = env_run<T, CPLX>(in, nullptr, w0, s0, e, g);
    ends[c] = env_run<T, CPLX>(in, out, s0, s1, e, g);
}

template <typename T, bool CPLX>
__global__ __launch_bounds__(kNT) void env_repair_kernel(const T *__restrict__ in, float *__restrict__ out, int64_t n, int64_t C,
                                                          int64_t nch, const float *__restrict__ ends, unsigned char *__restrict__ miss,
                                                          unsigned long long *__restrict__ cnt, EnvGains g)
{
    const int64_t c = (int64_t)blockIdx.x * kNT + threadIdx.x + 1;
    bool rewrote = false, suspect = false;
    if (c < nch) {
        const int64_t s0 = c * C, s1 = s0 + C < n ? s0 + C : n;
        const bool matched = env_mend<T, CPLX>(in, out, s0, s1, ends[c - 1], g, &rewrote);
        miss[c] = matched ? 0 : 1;
        suspect = !matched && c + 1 < nch;
    }
    const unsigned long long r = __ballot(rewrote), s = __ballot(suspect);
    if ((threadIdx.x & 63) == 0) {
        if (r) atomicAdd(&cnt[kRepaired], (unsigned long long)__popcll(r));
        if (s) atomicAdd(&cnt[kSuspect], (unsigned long long)__popcll(s));
    }
}

template <typename T, bool CPLX>
__global__ __launch_bounds__(64) void env_resolve_kernel(const T *__restrict__ in, float *__restrict__ out, int64_t n, int64_t C,
                                                         int64_t nch, const unsigned char *__restrict__ miss,
                                                         unsigned long long *__restrict__ cnt, float *__restrict__ state, EnvGains g)
{
    if (threadIdx.x != 0) return;
    if (cnt[kSuspect] != 0) {
        bool carry = false;
        unsigned long long resolved = 0;
        for (int64_t c = 1; c < nch; c++) {
            if (!carry && !(c >= 2 && miss[c - 1])) continue;
            const int64_t s0 = c * C, s1 = s0 + C < n ? s0 + C : n;
            bool rewrote = false;
            carry = !env_mend<T, CPLX>(in, out, s0, s1, out[s0 - 1], g, &rewrote);
            resolved++;
        }
        cnt[kResolved] += resolved;
    }
    *state = out[n - 1];
}

template <typename T, bool CPLX>
int slice_t(const EnvShape &p, const void *in, float *out, size_t n, float *state, float *ends, unsigned char *miss,
            unsigned long long *cnt, bool first, hipStream_t st)
{
    const int64_t nch = (int64_t)((n + p.C - 1) / p.C);
    const unsigned g1 = (unsigned)((nch + kNT - 1) / kNT);
    const unsigned g2 = (unsigned)(nch > 1 ? (nch - 1 + kNT - 1) / kNT : 1);
    hipLaunchKernelGGL((env_spec_kernel<T, CPLX>), dim3(g1), dim3(kNT), 0, st, (const T *)in, out, (int64_t)n, (int64_t)p.C,
                       (int64_t)p.W, nch, (const float *)state, ends, cnt, first ? 1 : 0, p.g);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((env_repair_kernel<T, CPLX>), dim3(g2), dim3(kNT), 0, st, (const T *)in, out, (int64_t)n, (int64_t)p.C, nch,
                       (const float *)ends, miss, cnt, p.g);
    PCX_LAUNCH_CHECK();
    hipLaunchKernelGGL((env_resolve_kernel<T, CPLX>), dim3(1), dim3(64), 0, st, (const T *)in, out, (int64_t)n, (int64_t)p.C, nch,
                       (const unsigned char *)miss, cnt, state, p.g);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace

int launch_envelope_slice(const EnvShape &p, const void *in, float *out, size_t n, float *state, float *ends, unsigned char *miss,
                          unsigned long long *cnt, bool first, hipStream_t st)
{
    if (n == 0) return PCX_OK;
    switch (p.scalar * 2 + (p.cplx ? 1 : 0)) {
    case PCX_F64 * 2: return slice_t<double, false>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_F64 * 2 + 1: return slice_t<double, true>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_F32 * 2: return slice_t<float, false>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_F32 * 2 + 1: return slice_t<float, true>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I64 * 2: return slice_t<int64_t, false>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I64 * 2 + 1: return slice_t<int64_t, true>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I32 * 2: return slice_t<int32_t, false>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I32 * 2 + 1: return slice_t<int32_t, true>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I16 * 2: return slice_t<int16_t, false>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I16 * 2 + 1: return slice_t<int16_t, true>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I8 * 2: return slice_t<int8_t, false>(p, in, out, n, state, ends, miss, cnt, first, st);
    case PCX_I8 * 2 + 1: return slice_t<int8_t, true>(p, in, out, n, state, ends, miss, cnt, first, st);
    }
    set_error("envelope_detector: unsupported type (scalar %d)", p.scalar);
    return PCX_ERR_ARG;
}

}  // namespace pcx
