// framesync.hip -- /comms/frame_sync (digital/FrameSync.cpp): the search for the sync word of /comms/frame_insert and the recovery of
// the payload behind it.  Four kernels:
//   metric   for every candidate offset i of a call the reference's three steps (:596-693): the envelope check, the frequency estimate
//            and the frequency-corrected correlation L over the W samples of the sync word; it writes corrPeak = trunc(|L|), 4 bytes per
//            offset.  A lane owns an offset.  The envelope gate reads the stream directly (two loads per offset on silence) and a
//            workgroup without a single open gate leaves; otherwise the W samples pass through LDS in chunks of kChunk, a tile of kTile
//            offsets and its halo at a time, and lane t reads element t + j of the chunk: consecutive lanes, consecutive addresses.
//            A launch covers the offsets [first, N) of a call; first is a multiple of kTile, so the tiles of a call never move.
//   scan     the reference's peak tracker (:488-502) over the corrPeak words: a running strict maximum that carries the index of its
//            first occurrence (associative: a scan), then the first offset at which that maximum has stood for corrDurThresh offsets (a
//            minimum).  One workgroup, from a carried (maxPeak, countSinceMax).  While no maximum stands it walks the metric kernel's
//            per-tile flags (does the tile hold a corrPeak above the threshold) instead of the words: 256 Ki offsets a step.
//   finish   one wave: the three estimates at the peak, by the device functions of the metric kernel on that one offset in the same
//            order of operations (the bits the search saw), then the first-bit search (:709-721) and the 58 header bits as one word.
//   payload  out = in * scale (RAW), in * polar(scale, phase0 + k inc) (PHASE, DEBUG), in[k dw] * polar(scale, phase0 + k inc dw)
//            (TIMING): the phase in closed form, 16-byte accesses where the addresses allow.
// ALL ARITHMETIC IS DOUBLE, for complex_float32 streams too: the decisions hang on trunc(|L|) and on comparisons of nearly equal
// values, and a float32 sum over W terms moves |L| by 1e-5 W.  The rotation exp(i deltaFc j) advances by a complex multiply and is set
// afresh from sincos every kAnchor samples.  Nothing is kept in private memory; no atomics besides one LDS minimum in the scan.
#include "pcx_internal.hpp"
#include "vec_io.hpp"

namespace pcx {
namespace {

constexpr int kTile = 256;                  // offsets of a workgroup of the metric kernel, one per lane
constexpr int kChunk = 768;                 // samples of the sync word staged at a time (a multiple of kAnchor)
constexpr int kStage = kChunk + kTile;      // elements in LDS: 8 KiB (complex_float32), 16 KiB (complex_float64)
constexpr int kAnchor = 16;                 // the rotation is set from sincos at every multiple of this
constexpr int kScanThreads = 1024;
constexpr int kScanRun = 16;                // consecutive offsets a thread of the scan owns
constexpr uint64_t kNone = ~(uint64_t)0;
static_assert(kChunk % kAnchor == 0 && (kAnchor & (kAnchor - 1)) == 0, "chunks begin at an anchor");

struct C2 {
    double re, im;
};
__device__ __forceinline__ double cabs2(const C2 &a) { return hypot(a.re, a.im); }

// where an offset's samples come from: sample j of the window
template <typename T>
struct GlobalAt {                           // the call's buffer
    const Vec<T, 2> *p;
    __device__ __forceinline__ C2 operator()(size_t j) const
    {
        const Vec<T, 2> v = p[j];
        return C2{(double)v.v[0], (double)v.v[1]};
    }
};
template <typename T>
struct LdsAt {                              // the staged chunk: element 0 is sample c0 of the tile's first offset
    const Vec<T, 2> *p;
    size_t c0;
    __device__ __forceinline__ C2 operator()(size_t j) const
    {
        const Vec<T, 2> v = p[j - c0];
        return C2{(double)v.v[0], (double)v.v[1]};
    }
};
template <typename T>
struct VirtAt {                             // the call's buffer from a signed offset: zeros outside of it (a guard: see the finish kernel)
    const Vec<T, 2> *x;
    size_t n;
    int64_t base;
    __device__ __forceinline__ C2 operator()(size_t j) const
    {
        const int64_t idx = base + (int64_t)j;
        Vec<T, 2> v;
        v.v[0] = v.v[1] = 0;
        if (idx >= 0 && (uint64_t)idx < n) v = x[idx];
        return C2{(double)v.v[0], (double)v.v[1]};
    }
};

// processEnvelope (:596-634): 0 when the gate stays shut
template <typename At>
__device__ __forceinline__ double envelope(const FsyncShape &s, At at)
{
    if (cabs2(at(s.dw)) < s.thresh) return 0;
    if (cabs2(at(s.W - s.dw)) < s.thresh) return 0;
    const size_t half = s.sw * s.dw / 2;
    double sum0 = 0;
    for (size_t i = s.dw; i < half; i++) sum0 += cabs2(at(i));
    sum0 /= (double)(half - s.dw);
    if (sum0 < s.thresh) return 0;
    sum0 /= s.abs_front;
    double sum1 = 0;
    for (size_t i = s.W - half; i < s.W - s.dw; i++) sum1 += cabs2(at(i));
    sum1 /= (double)(half - s.dw);
    if (sum1 < s.thresh) return 0;
    sum1 /= s.abs_back;
    const double ratio = sum0 / sum1;
    if (ratio > 2 || ratio < 0.5) return 0;
    return 2.0 / (sum0 + sum1);
}

// processFreqSync (:639-664)
template <typename At>
__device__ __forceinline__ double freq_sync(const FsyncShape &s, At at)
{
    const size_t width = s.sw * s.dw, base = width * (s.P - 1), delta = width / 2;
    const size_t end = width - delta - s.dw;
    double kre = 0, kim = 0;
    for (size_t i = s.dw; i < end; i++) {
        const C2 a = at(base + i), b = at(base + i + delta);
        kre += a.re * b.re + a.im * b.im;           // a * conj(b)
        kim += a.im * b.re - a.re * b.im;
    }
    return atan2(kim, kre) / (double)delta;
}

// processSyncWord (:669-693) as sum over the symbols s of conj(preamble[s]) * sum over its samples of x[j] exp(i deltaFc j), times scale
struct Corr {
    double lre = 0, lim = 0, sre = 0, sim = 0, rre = 1, rim = 0, stre = 1, stim = 0, dfc = 0;
    size_t left = 0, sym = 0;
};
__device__ __forceinline__ void corr_begin(Corr &c, double dfc, size_t width)
{
    c.dfc = dfc;
    sincos(dfc, &c.stim, &c.stre);
    c.left = width;
}
template <typename At>
__device__ __forceinline__ void corr_span(Corr &c, const FsyncShape &s, const C2 *pre, size_t j0, size_t j1, At at)
{
    const size_t width = s.sw * s.dw;
    for (size_t j = j0; j < j1; j++) {
        if ((j & (kAnchor - 1)) == 0) sincos(c.dfc * (double)j, &c.rim, &c.rre);
        const C2 x = at(j);
        c.sre += x.re * c.rre - x.im * c.rim;
        c.sim += x.re * c.rim + x.im * c.rre;
        const double nre = c.rre * c.stre - c.rim * c.stim, nim = c.rre * c.stim + c.rim * c.stre;
        c.rre = nre;
        c.rim = nim;
        if (--c.left == 0) {
            const C2 p = pre[c.sym];
            c.lre += p.re * c.sre + p.im * c.sim;   // conj(p) * S
            c.lim += p.re * c.sim - p.im * c.sre;
            c.sre = c.sim = 0;
            c.sym++;
            c.left = width;
        }
    }
}
// trunc(|L|) as 32 bits; a magnitude that is not a number counts as no correlation
__device__ __forceinline__ uint32_t corr_peak(const Corr &c, double scale, double *phase_off)
{
    const double re = c.lre * scale, im = c.lim * scale;
    *phase_off = -atan2(im, re);
    const double mag = hypot(re, im);
    if (!(mag >= 0)) return 0;
    return mag < 4294967295.0 ? (uint32_t)mag : 0xffffffffu;
}

template <typename T>
__global__ __launch_bounds__(kTile) void fsync_metric_kernel(const Vec<T, 2> *__restrict__ x, size_t n, size_t first, size_t N, FsyncShape s,
                                                             const C2 *__restrict__ pre, uint32_t thresh, uint32_t *__restrict__ peaks, uint32_t *__restrict__ flags)
{
    __shared__ Vec<T, 2> stage[kStage];
    const size_t tile0 = first + (size_t)blockIdx.x * kTile, i = tile0 + threadIdx.x;
    const bool active = i < N;
    double scale = 0, dfc = 0;
    if (active) {
        const GlobalAt<T> at{x + i};
        scale = envelope(s, at);
        if (scale != 0) dfc = freq_sync(s, at);
    }
    if (!__syncthreads_or(scale != 0)) {
        if (active) peaks[i] = 0;
        if (threadIdx.x == 0) flags[tile0 / kTile] = 0;
        return;
    }
    Corr c;
    corr_begin(c, dfc, s.sw * s.dw);
    for (size_t c0 = 0; c0 < s.W; c0 += kChunk) {
        const size_t c1 = c0 + kChunk < s.W ? c0 + kChunk : s.W, need = c1 - c0 + kTile - 1;
        if (c0) __syncthreads();
        for (size_t k = threadIdx.x; k < need; k += kTile) {
            const size_t g = tile0 + c0 + k;
            Vec<T, 2> v;
            v.v[0] = v.v[1] = 0;
            if (g < n) v = x[g];
            stage[k] = v;
        }
        __syncthreads();
        if (scale != 0) corr_span(c, s, pre, c0, c1, LdsAt<T>{stage + threadIdx.x, c0});
    }
    double phase_off;
    const uint32_t peak = active && scale != 0 ? corr_peak(c, scale, &phase_off) : 0;
    if (active) peaks[i] = peak;
    // does the tile hold an offset the tracker would take for a new maximum at all
    const int any = __syncthreads_or(peak > thresh);
    if (threadIdx.x == 0) flags[tile0 / kTile] = any;
}

// ---- the peak tracker
struct Rec {                                // a running strict maximum and where it first stood (kNone: not in this launch)
    uint32_t v;
    uint64_t at;
};
__device__ __forceinline__ Rec later(const Rec &a, const Rec &b) { return b.v > a.v ? b : a; }

__global__ __launch_bounds__(kScanThreads) void fsync_scan_kernel(const uint32_t *__restrict__ peaks, const uint32_t *__restrict__ flags, uint64_t s0, uint64_t N,
                                                                  uint32_t thresh, uint64_t dur, uint32_t max0, uint64_t cnt0, FsyncScanOut *out)
{
    __shared__ uint32_t sv[kScanThreads];
    __shared__ uint64_t sa[kScanThreads];
    __shared__ unsigned long long found, skipto;
    const unsigned tid = threadIdx.x;
    const uint64_t ntiles = (N + kTile - 1) / kTile;
    Rec carry{max0, kNone};
    if (tid == 0) found = kNone;
    for (uint64_t base = s0; base < N; base += (uint64_t)kScanThreads * kScanRun) {
        if (carry.v < thresh) {
            // no maximum stands (the same in every thread): nothing is declared in front of the next offset above the threshold, and
            // the count in front of it is a function of the offset alone.  Go on at the first tile that holds such an offset
            __syncthreads();
            if (tid == 0) skipto = kNone;
            __syncthreads();
            for (uint64_t t0 = base / kTile; t0 < ntiles; t0 += kScanThreads) {
                const bool set = t0 + tid < ntiles && flags[t0 + tid] != 0;
                if (set) atomicMin(&skipto, (unsigned long long)(t0 + tid));
                if (__syncthreads_or(set)) break;
            }
            const uint64_t tile = skipto;
            if (tile == kNone) break;
            if (tile * kTile > base) base = tile * kTile;
        }
        const uint64_t a = base + (uint64_t)tid * kScanRun, b = a + kScanRun < N ? a + kScanRun : N;
        Rec mine{0, kNone};
        for (uint64_t k = a; k < b; k++) {
            const uint32_t v = peaks[k];
            if (v > thresh && v > mine.v) mine = Rec{v, k};
        }
        __syncthreads();                    // the previous round's reads of sv / sa, and `found` set
        sv[tid] = mine.v;
        sa[tid] = mine.at;
        __syncthreads();
        for (unsigned d = 1; d < kScanThreads; d <<= 1) {       // inclusive scan, earlier element on the left
            Rec r{sv[tid], sa[tid]};
            if (tid >= d) r = later(Rec{sv[tid - d], sa[tid - d]}, r);
            __syncthreads();
            sv[tid] = r.v;
            sa[tid] = r.at;
            __syncthreads();
        }
        Rec m = tid ? later(carry, Rec{sv[tid - 1], sa[tid - 1]}) : carry;
        const Rec last = later(carry, Rec{sv[kScanThreads - 1], sa[kScanThreads - 1]});
        uint64_t hit = kNone, hit_cnt = 0;
        Rec hit_m = m;
        for (uint64_t k = a; k < b; k++) {
            const uint32_t v = peaks[k];
            if (v > m.v && v > thresh) m = Rec{v, k};
            const uint64_t cnt = m.at != kNone ? k - m.at + 1 : cnt0 + (k - s0 + 1);
            if (m.v >= thresh && cnt >= dur) {
                hit = k;
                hit_cnt = cnt;
                hit_m = m;
                break;
            }
        }
        if (hit != kNone) atomicMin(&found, (unsigned long long)hit);
        __syncthreads();
        if (found != kNone) {
            if (hit == found) {
                out->declared = 1;
                out->at = hit;
                out->max_peak = hit_m.v;
                out->count = hit_cnt;
                out->peak_idx = hit_m.at;
            }
            return;
        }
        carry = last;
    }
    if (tid == 0) {
        out->declared = 0;
        out->at = N;
        out->max_peak = carry.v;
        out->count = carry.at != kNone ? N - carry.at : cnt0 + (N > s0 ? N - s0 : 0);
        out->peak_idx = carry.at;
    }
}

// ---- estimates at the peak, first-bit search, header bits: one wave
template <typename T>
__global__ __launch_bounds__(64) void fsync_finish_kernel(const Vec<T, 2> *x, size_t n, FsyncShape s, const C2 *pre,
                                                          FsyncEst carried, const FsyncScanOut *scan, FsyncFinishOut *out)
{
    // what the tracker left: a maximum of this launch is estimated afresh, a carried one keeps its estimates; a declared frame begins
    // `count` offsets in front of the offset behind the declaring one
    const bool do_est = scan->peak_idx != kNone, do_header = scan->declared != 0;
    // (frame_off is one element in front of the peak and may lie up to corrDurThresh elements in front of the buffer, when the peak was
    // in the previous call.  Nothing is read there: the first element the header search reads is frame_off + W - sw dw / 2, at or behind
    // the declaring offset because W - sw dw / 2 >= W / 2 >= corrDurThresh.  VirtAt's zeros outside of the buffer are a guard.)
    const int64_t peak = (int64_t)scan->peak_idx, frame_off = (int64_t)scan->at - (int64_t)scan->count;
    __shared__ double est[3];
    __shared__ double sv[64];
    __shared__ unsigned long long sfirst;
    __shared__ int sdone, sfound;
    const unsigned lane = threadIdx.x;
    if (lane == 0) {
        FsyncEst e = carried;
        if (do_est) {
            const VirtAt<T> at{x, n, peak};
            e.scale = envelope(s, at);
            e.delta_fc = e.phase_off = 0;
            if (e.scale != 0) {
                e.delta_fc = freq_sync(s, at);
                Corr c;
                corr_begin(c, e.delta_fc, s.sw * s.dw);
                corr_span(c, s, pre, 0, s.W, at);
                (void)corr_peak(c, e.scale, &e.phase_off);
            }
        }
        est[0] = e.scale;
        est[1] = e.delta_fc;
        est[2] = e.phase_off;
        out->scale = e.scale;
        out->delta_fc = e.delta_fc;
        out->phase_off = e.phase_off;
        out->first_bit = 0;
        out->bits = 0;
        out->found = 0;
        sdone = 0;
    }
    __syncthreads();
    if (!do_header) return;
    const double scale = est[0], dfc = est[1], poff = est[2];
    const VirtAt<T> at{x, n, frame_off};
    const C2 last = pre[s.P - 1];
    // Re(x * polar(scale, phase) * conj(last symbol))
    auto bit_value = [&](size_t k, double phase) {
        const C2 v = at(k);
        double sn, cs;
        sincos(phase, &sn, &cs);
        const double pr = scale * cs, pi = scale * sn;
        const double bre = v.re * pr - v.im * pi, bim = v.re * pi + v.im * pr;
        return bre * last.re + bim * last.im;
    };
    // the first-bit search: 64 values at a time, walked in order by lane 0
    size_t first = s.W + s.dw / 2;
    double fpeak = 0;
    for (size_t k0 = s.W - s.sw * s.dw / 2; k0 < s.F; k0 += 64) {
        const size_t k = k0 + lane;
        sv[lane] = k < s.F ? bit_value(k, poff + dfc * (double)k) : 0.0;
        __syncthreads();
        if (lane == 0) {
            for (unsigned l = 0; l < 64 && k0 + l < s.F; l++) {
                const double v = sv[l];
                if (v > fpeak) {
                    if (fpeak == 0) continue;
                    sdone = 1;
                    break;
                }
                first = k0 + l;
                fpeak = v;
            }
        }
        __syncthreads();
        if (sdone) break;
    }
    if (lane == 0) {
        sfirst = first;
        sfound = fpeak != 0;            // (a peak that is not a number counts as found: its bits are all 0)
    }
    __syncthreads();
    if (!sfound) return;
    first = sfirst;
    const bool one = lane < PCX_FRAME_HEADER_BITS && bit_value(first + lane * s.dw, (poff + dfc * (double)first) + (double)lane * (dfc * (double)s.dw)) > 0;
    const unsigned long long word = __ballot(one);
    if (lane == 0) {
        out->first_bit = first;
        out->bits = word;
        out->found = 1;
    }
}

// ---- the payload
template <typename T>
__device__ __forceinline__ void turn(const T *in, T *out, double pr, double pi)
{
    const double re = in[0], im = in[1];
    out[0] = (T)(re * pr - im * pi);
    out[1] = (T)(re * pi + im * pr);
}
// MODE 0: RAW, 1: PHASE, 2: TIMING; V: elements of one access (2: complex_float32 at 16-byte aligned addresses)
template <typename T, int MODE, int V>
__global__ __launch_bounds__(256) void fsync_payload_kernel(const Vec<T, 2> *__restrict__ in, Vec<T, 2> *__restrict__ out, size_t N, size_t dw, double scale,
                                                            double phase0, double inc)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    auto factor = [&](size_t k, double *pr, double *pi) {
        if (MODE == 0) {
            *pr = scale;
            *pi = 0;
        } else {
            double sn, cs;
            sincos(phase0 + (double)k * inc, &sn, &cs);
            *pr = scale * cs;
            *pi = scale * sn;
        }
    };
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u * V < N; u += stride) {
        const size_t e = u * V;
        double pr, pi;
        if constexpr (V == 2) if (e + 1 < N) {
            Vec<T, 4> a = nt_load(reinterpret_cast<const Vec<T, 4> *>(in + e)), r;
            factor(e, &pr, &pi);
            if (MODE == 0) { r.v[0] = (T)((double)a.v[0] * pr); r.v[1] = (T)((double)a.v[1] * pr); }
            else turn(&a.v[0], &r.v[0], pr, pi);
            factor(e + 1, &pr, &pi);
            if (MODE == 0) { r.v[2] = (T)((double)a.v[2] * pr); r.v[3] = (T)((double)a.v[3] * pr); }
            else turn(&a.v[2], &r.v[2], pr, pi);
            nt_store(reinterpret_cast<Vec<T, 4> *>(out + e), r);
            continue;
        }
        {
            const Vec<T, 2> a = MODE == 2 ? in[e * dw] : nt_load(in + e);
            Vec<T, 2> r;
            factor(e, &pr, &pi);
            if (MODE == 0) { r.v[0] = (T)((double)a.v[0] * pr); r.v[1] = (T)((double)a.v[1] * pr); }
            else turn(&a.v[0], &r.v[0], pr, pi);
            nt_store(out + e, r);
        }
    }
}

}  // namespace

size_t fsync_tile() { return kTile; }

int launch_fsync_metric(const FsyncShape &s, const void *x, size_t n, size_t first, size_t N, const double *pre, uint32_t thresh, uint32_t *peaks,
                        uint32_t *flags, hipStream_t st)
{
    if (n < s.F || N > n - s.F + 1 || first >= N) return PCX_OK;
    const size_t grid = (N - first + kTile - 1) / kTile;
    if (grid > 0x7fffffffu) { set_error("frame sync: %zu offsets in one launch", N - first); return PCX_ERR_ARG; }
    const C2 *p = reinterpret_cast<const C2 *>(pre);
    if (s.f64) hipLaunchKernelGGL(fsync_metric_kernel<double>, dim3((unsigned)grid), dim3(kTile), 0, st, static_cast<const Vec<double, 2> *>(x), n, first, N, s, p, thresh, peaks, flags);
    else hipLaunchKernelGGL(fsync_metric_kernel<float>, dim3((unsigned)grid), dim3(kTile), 0, st, static_cast<const Vec<float, 2> *>(x), n, first, N, s, p, thresh, peaks, flags);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

int launch_fsync_scan(const uint32_t *peaks, const uint32_t *flags, uint64_t s0, uint64_t N, uint32_t thresh, uint64_t dur, uint32_t max0, uint64_t cnt0,
                      FsyncScanOut *out, hipStream_t st)
{
    hipLaunchKernelGGL(fsync_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, peaks, flags, s0, N, thresh, dur, max0, cnt0, out);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

int launch_fsync_finish(const FsyncShape &s, const void *x, size_t n, const double *pre, const FsyncEst &carried,
                        const FsyncScanOut *scan, FsyncFinishOut *out, hipStream_t st)
{
    const C2 *p = reinterpret_cast<const C2 *>(pre);
    if (s.f64)
        hipLaunchKernelGGL(fsync_finish_kernel<double>, dim3(1), dim3(64), 0, st, static_cast<const Vec<double, 2> *>(x), n, s, p, carried, scan,
                           out);
    else
        hipLaunchKernelGGL(fsync_finish_kernel<float>, dim3(1), dim3(64), 0, st, static_cast<const Vec<float, 2> *>(x), n, s, p, carried, scan,
                           out);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

namespace {
template <typename T, int MODE, int V>
void payload_launch(const void *in, void *out, size_t N, size_t dw, double scale, double phase0, double inc, hipStream_t st)
{
    hipLaunchKernelGGL((fsync_payload_kernel<T, MODE, V>), dim3(stream_grid((N + V - 1) / V, 256)), dim3(256), 0, st, static_cast<const Vec<T, 2> *>(in),
                       static_cast<Vec<T, 2> *>(out), N, dw, scale, phase0, inc);
}
template <typename T, int V>
void payload_mode(int mode, const void *in, void *out, size_t N, size_t dw, double scale, double phase0, double inc, hipStream_t st)
{
    if (mode == 0) payload_launch<T, 0, V>(in, out, N, dw, scale, phase0, inc, st);
    else if (mode == 1) payload_launch<T, 1, V>(in, out, N, dw, scale, phase0, inc, st);
    else payload_launch<T, 2, 1>(in, out, N, dw, scale, phase0, inc, st);
}
}  // namespace

// mode 0: RAW, 1: PHASE / DEBUG, 2: TIMING (inc: the phase step from one OUTPUT element to the next)
int launch_fsync_payload(bool f64, int mode, const void *in, void *out, size_t N, size_t dw, double scale, double phase0, double inc, hipStream_t st)
{
    if (!N) return PCX_OK;
    if (f64) payload_mode<double, 1>(mode, in, out, N, dw, scale, phase0, inc, st);
    else if ((((uintptr_t)in | (uintptr_t)out) & 15) == 0) payload_mode<float, 2>(mode, in, out, N, dw, scale, phase0, inc, st);
    else payload_mode<float, 1>(mode, in, out, N, dw, scale, phase0, inc, st);
    PCX_LAUNCH_CHECK();
    return PCX_OK;
}

}  // namespace pcx
