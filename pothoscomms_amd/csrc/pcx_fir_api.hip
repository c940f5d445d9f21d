// pcx_fir_api.hip -- the extern "C" boundary (include/pcx.h), part 2: /comms/fir_filter (pcx_fir_*) and the fused
// Rotate -> FIR -> FreqDemod chain (pcx_fmchain_*): tap bookkeeping (FIRFilter.cpp:138-173,327-354), the coefficient tables of
// the handle's plan (fir_plan.hpp chooses it), host-buffer calls.  Host-side only.
#include "pcx_host.hpp"
#include "pcx_tables.hpp"
#include "fir_plan.hpp"

using namespace pcx;

/* ===================================================================== *
 *  FIR
 * ===================================================================== */
struct pcx_fir {
    ExecCtx cx;
    int scalar = PCX_F32, cplx = 1, ctaps = 1;
    std::vector<double> taps;  // ntaps * (ctaps ? 2 : 1)
    size_t ntaps = 1, M = 1, L = 1, K = 1, inputRequire = 1;
    int algo = PCX_FIR_AUTO, last_algo = 0, last_plan = PCX_FIR_PLAN_NONE;
    QFormat qf = kDefaultQFormat;   // integer element types: the floatToQ / fromQ reading (pcx_fir_set_qformat; the process-wide one at creation)
    bool dirty = true;
    FirPlan plan;             // which plan serves these settings (fir_plan.hpp), set with the tables: valid while !dirty
    DevBuf rowLen, rowTaps, tapsRev;   // the time-domain kernels' tables
    // the frequency-domain plan's tables: Hspec one spectrum (or the partitions' spectra) of the whole tap vector, HspecRows / HrowsD one
    // per polyphase row in float / double, Hdecim the lane-ordered spectrum of the folded (CF32_DECIM) and replicated (CF32_INTERP) forms
    DevBuf Hspec, HspecRows, HrowsD, Hdecim, tw4096;
    StageBuf wsIn, wsOut;
    DevBuf wsRows;            // the row plans: one contiguous output row per polyphase row, interleaved afterwards
    DevBuf sched;             // SchedState: dynamic block assignment of the overlap-save kernels (pcx_sched.hpp), zeroed once
    unsigned slots = 1024;    // resident workgroups a persistent launch may take (pcx_shard: several shards on one device share it)
    size_t lead_valid = 0;    // set around the chunks of a drained host call: samples of the same stream in front of the chunk's first
    size_t Kp = 8;
    bool taps24 = false;      // integer Q taps all fit 24 signed bits (v_mul_i32_i24 path)
    bool taps16 = false;      // complex_int16 / complex_int8 stream, complex taps within +-32767 after floatToQ (v_dot2_i32_i16 path)
    DevBuf tapsP;             // packed (a, -b), (b, a) pairs for that path
};

constexpr size_t kRowsWorkspaceCap = (size_t)1 << 30;   // polyphase-row workspace of the interpolating paths (pcx_fir_process_dev)

// FIRFilter::updateInternals, FIRFilter.cpp:327-354 (host mirror; tables uploaded lazily)
static void fir_update_internals(pcx_fir *h)
{
    h->K = h->ntaps / h->L + ((h->ntaps % h->L) == 0 ? 0 : 1);
    h->inputRequire = h->M + (h->K - 1);
    h->dirty = true;
}

template <typename TT>
static int fir_upload_rows(pcx_fir *h, bool integer)
{
    const size_t L = h->L, K = h->K, w = h->ctaps ? 2 : 1;
    std::vector<uint32_t> rowLen(L, 0);
    std::vector<TT> rows(L * K * w, TT(0));
    for (size_t j = 0; j < L; j++) {
        size_t len = 0;
        for (size_t k = 0; k < K; k++) {
            const size_t i = j + k * L;
            if (i >= h->ntaps) continue;
            for (size_t c = 0; c < w; c++) {
                const double t = h->taps[i * w + c];
                rows[(j * K + len) * w + c] = integer ? (TT)float_to_q(t, h->scalar, h->qf) : (TT)t;  // floatToQ<QTapsType>, :348
            }
            len++;
        }
        rowLen[j] = (uint32_t)len;
    }
    PCX_TRY(upload(h->rowLen, rowLen));
    PCX_TRY(upload(h->rowTaps, rows));
    h->taps24 = integer;
    if (integer)
        for (const TT &t : rows)
            if ((long long)t < -(1ll << 23) || (long long)t >= (1ll << 23)) { h->taps24 = false; break; }
    h->taps16 = false;
    if (integer && (h->scalar == PCX_I16 || h->scalar == PCX_I8) && h->cplx && h->ctaps && L == 1 && h->M == 1) {
        bool ok = true;
        for (const TT &t : rows)
            if ((long long)t < -32767 || (long long)t > 32767) { ok = false; break; }
        if (ok) {
            std::vector<uint32_t> packed(2 * K);
            for (size_t k = 0; k < K; k++) {
                const uint32_t a = (uint16_t)(int16_t)rows[2 * k], b = (uint16_t)(int16_t)rows[2 * k + 1];
                const uint32_t nb = (uint16_t)(int16_t)(-(long long)rows[2 * k + 1]);
                packed[2 * k] = a | (nb << 16);        // (a, -b): real part
                packed[2 * k + 1] = b | (a << 16);     // (b,  a): imaginary part
            }
            PCX_TRY(upload(h->tapsP, packed));
            h->taps16 = true;
        }
    }
    return PCX_OK;
}

// Tap i as the frequency-domain pipeline of the element type sees it (floatToQ<QTapsType>, FIRFilter.cpp:348): float64 as it is, float32
// narrowed to float first, int16 / int8 the Q-format taps exactly as the time-domain kernels use them (int32 / int16).  As a double.
static std::complex<double> fir_tap(const pcx_fir *h, size_t i)
{
    auto q = [&](double t) -> double {
        switch (h->scalar) {
        case PCX_F64: return t;
        case PCX_F32: return (double)(float)t;
        case PCX_I16: return (double)(int32_t)float_to_q(t, h->scalar, h->qf);
        default: return (double)(int16_t)float_to_q(t, h->scalar, h->qf);
        }
    };
    return h->ctaps ? std::complex<double>(q(h->taps[2 * i]), q(h->taps[2 * i + 1])) : std::complex<double>(q(h->taps[i]), 0.0);
}

// Row j of L polyphase rows, h_j[k] = taps[j + k L] (FIRFilter.cpp:341-350); L = 1: the whole tap vector.  A row the tap vector
// leaves short is simply shorter, and empty where L > ntaps: every table builder sums the taps it is given into zeros, so trailing
// zero taps (or a single zero for an empty row) change no byte of a table.
static std::vector<std::complex<double>> fir_row(const pcx_fir *h, size_t j, size_t L)
{
    std::vector<std::complex<double>> row;
    for (size_t i = j; i < h->ntaps; i += L) row.push_back(fir_tap(h, i));
    return row;
}

// one table per polyphase row of the handle, `per_row` entries apart
template <typename T, typename Make>
static std::vector<T> fir_row_tables(const pcx_fir *h, size_t per_row, Make &&make)
{
    std::vector<T> rows(h->L * per_row);
    for (size_t j = 0; j < h->L; j++) {
        const std::vector<T> t = make(fir_row(h, j, h->L));
        std::copy(t.begin(), t.end(), rows.begin() + j * per_row);
    }
    return rows;
}

// int16 / int8: the double transform reproduces the integer convolution bit for bit while ||h_q||_2 < 2^22 (fir_ols_f64.hip), held for
// every polyphase row (L = 1: the whole tap vector)
static bool fir_taps_exact(const pcx_fir *h)
{
    if (h->scalar != PCX_I16 && h->scalar != PCX_I8) return true;
    for (size_t j = 0; j < h->L && j < h->ntaps; j++) {
        double norm2 = 0;
        for (const std::complex<double> &t : fir_row(h, j, h->L)) norm2 += std::norm(t);
        if (norm2 >= 17592186044416.0) return false;   // 2^44
    }
    return true;
}

static int fir_sync_tables(pcx_fir *h)
{
    if (!h->dirty) return PCX_OK;
    PCX_TRY(ctx_quiesce(h->cx));   // a kernel of an earlier call may still be reading the tables rewritten below
    switch (h->scalar) {
    case PCX_F32: PCX_TRY(fir_upload_rows<float>(h, false)); break;
    case PCX_F64: PCX_TRY(fir_upload_rows<double>(h, false)); break;
    case PCX_I64: case PCX_I32: PCX_TRY(fir_upload_rows<int64_t>(h, true)); break;
    case PCX_I16: PCX_TRY(fir_upload_rows<int32_t>(h, true)); break;
    case PCX_I8: PCX_TRY(fir_upload_rows<int16_t>(h, true)); break;
    }
    if (!h->sched.p) {
        PCX_TRY(h->sched.ensure_zeroed(kSchedBytes));
    }
    if (h->scalar == PCX_F32 && h->cplx && h->M == 1 && h->L == 1) {
        const size_t K = h->K;
        // reversed, zero-padded complex taps for the LDS-tiled direct kernel
        h->Kp = (K + 7) / 8 * 8;
        std::vector<float> rev(2 * h->Kp, 0.f);
        for (size_t m = 0; m < K; m++) {
            const size_t k = K - 1 - m;
            rev[2 * m] = (float)(h->ctaps ? h->taps[2 * k] : h->taps[k]);
            rev[2 * m + 1] = h->ctaps ? (float)h->taps[2 * k + 1] : 0.f;
        }
        PCX_TRY(upload(h->tapsRev, rev));
    }

    FirPlanIn in;
    in.scalar = h->scalar; in.cplx = h->cplx; in.ctaps = h->ctaps;
    in.ntaps = h->ntaps; in.L = h->L; in.M = h->M;
    in.taps16 = h->taps16;
    in.exact = fir_taps_exact(h);
    in.ols_int_min = (size_t)PCX_ENV_INT("PCX_OLS_INT_MIN", 0);
    in.ols_real_min = (size_t)PCX_ENV_INT("PCX_OLS_REAL_MIN", 0);
    in.ols64_n = (int)PCX_ENV_INT("PCX_OLS64_N", 0);
    in.decim_fullrate = PCX_ENV_SET("PCX_FIR_DECIM_FULLRATE");
    in.poly_strided = PCX_ENV_SET("PCX_FIR_POLY_STRIDED");
    in.slide = PCX_ENV_INT("PCX_FIR_SLIDE", 1) != 0;
    in.dot2 = PCX_ENV_INT("PCX_FIR_DOT2", 1) != 0;
    const FirPlan p = h->plan = fir_plan(in);

    // the tables of that plan and of no other
    const auto whole = [&] { return fir_row(h, 0, 1); };
    switch (p.ols_plan) {
    case PCX_FIR_PLAN_CF32_OLS4096: case PCX_FIR_PLAN_F32_OLS4096:
        PCX_TRY(upload(h->Hspec, make_hspec4096(whole())));
        PCX_TRY(upload(h->tw4096, make_tw4096()));
        break;
    case PCX_FIR_PLAN_CF32_UPOLS: case PCX_FIR_PLAN_F32_UPOLS: case PCX_FIR_PLAN_UPOLS_DECIM:
        PCX_TRY(upload(h->Hspec, make_hparts(whole(), p.parts)));
        PCX_TRY(upload(h->tw4096, make_tw4096()));
        break;
    case PCX_FIR_PLAN_UPOLS_ROWS:
        PCX_TRY(upload(h->HspecRows, fir_row_tables<float>(h, fir_upols_table_bytes(p.parts) / sizeof(float),
                                                           [&](const std::vector<std::complex<double>> &r) { return make_hparts(r, p.parts); })));
        PCX_TRY(upload(h->tw4096, make_tw4096()));
        break;
    case PCX_FIR_PLAN_F32_OLS4096_ROWS: case PCX_FIR_PLAN_CF32_OLS4096_ROWS: case PCX_FIR_PLAN_CF32_POLY:
        PCX_TRY(upload(h->HspecRows, fir_row_tables<float>(h, 2 * 4096, make_hspec4096)));
        PCX_TRY(upload(h->tw4096, make_tw4096()));
        break;
    case PCX_FIR_PLAN_CF32_DECIM:    // the decimator's phase: the output advanced by fold - 1 samples
        PCX_TRY(upload(h->Hdecim, turn_spectrum_lanes(make_hspec(whole(), 4096, p.fold - 1))));
        PCX_TRY(upload(h->tw4096, make_tw4096()));
        break;
    case PCX_FIR_PLAN_CF32_INTERP:   // H of the WHOLE tap vector, not of its rows
        PCX_TRY(upload(h->Hdecim, turn_spectrum_lanes(make_hspec(whole(), 4096))));
        PCX_TRY(upload(h->tw4096, make_tw4096()));
        break;
    case PCX_FIR_PLAN_CF64_OLS: case PCX_FIR_PLAN_REAL64_OLS:
        PCX_TRY(upload(h->Hspec, make_hspec<double>(whole(), (size_t)1 << p.log2n)));
        PCX_TRY(upload(h->tw4096, make_tw_ols64(p.log2n)));
        break;
    case PCX_FIR_PLAN_CF64_OLS_ROWS: case PCX_FIR_PLAN_REAL64_OLS_ROWS:
        PCX_TRY(upload(h->HrowsD, fir_row_tables<double>(h, 2 * 4096,
                                                         [](const std::vector<std::complex<double>> &r) { return make_hspec<double>(r, 4096); })));
        PCX_TRY(upload(h->tw4096, make_tw_ols64(p.log2n)));
        break;
    }
    h->dirty = false;
    return PCX_OK;
}


// (internal, pcx_shard.hip) upload the handle's tables now -- every allocation and transfer of the control plane -- instead of at its next call
namespace pcx {
int fir_prepare(pcx_fir *h)
{
    DeviceScope dev_scope(h->cx.device);
    return fir_sync_tables(h);
}
void fir_set_slots(pcx_fir *h, unsigned slots) { h->slots = slots; }
}  // namespace pcx

int pcx_fir_create(int scalar, int is_complex, int complex_taps, pcx_fir **out)
{
    PCX_CHECK_ARG(out, "null out");
    // FIRFilterFactory's if-chain, FIRFilter.cpp:371-383
    PCX_CHECK_ARG(valid_scalar(scalar), "FIRFilterFactory: unsupported types (scalar %d)", scalar);
    PCX_CHECK_ARG(!(complex_taps && !is_complex), "FIRFilterFactory: unsupported types (COMPLEX taps on a real stream)");
    pcx_fir *h = new (std::nothrow) pcx_fir();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->scalar = scalar; h->cplx = is_complex ? 1 : 0; h->ctaps = complex_taps ? 1 : 0;
    h->taps.assign(h->ctaps ? 2 : 1, 0.0);
    h->taps[0] = 1.0;  // ctor: setTaps({1}), FIRFilter.cpp:125
    h->ntaps = 1;
    h->qf = process_qformat();
    fir_update_internals(h);
    { DeviceScope bind(h->cx.device); }   // the handle belongs to the device current on the creating thread
    *out = h;
    return PCX_OK;
}
int pcx_fir_destroy(pcx_fir *h) { delete h; return PCX_OK; }
int pcx_fir_set_taps(pcx_fir *h, const double *taps, size_t ntaps)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(ntaps > 0 && taps, "FIRFilter::setTaps(): taps cannot be empty");
    h->taps.assign(taps, taps + ntaps * (h->ctaps ? 2 : 1));
    h->ntaps = ntaps;
    fir_update_internals(h);
    return PCX_OK;
}
int pcx_fir_set_decimation(pcx_fir *h, size_t decim)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(decim != 0, "FIRFilter::setDecimation(): decimation cannot be 0");
    h->M = decim;
    fir_update_internals(h);
    return PCX_OK;
}
int pcx_fir_set_interpolation(pcx_fir *h, size_t interp)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(interp != 0, "FIRFilter::setInterpolation(): interpolation cannot be 0");
    h->L = interp;
    fir_update_internals(h);
    return PCX_OK;
}
int pcx_fir_set_algo(pcx_fir *h, int algo)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(algo >= PCX_FIR_AUTO && algo <= PCX_FIR_EXACT, "unknown FIR algorithm %d", algo);
    h->algo = algo;
    return PCX_OK;
}
int pcx_fir_set_qformat(pcx_fir *h, const pcx_qformat *q)
{
    PCX_CHECK_ARG(h, "null handle");
    QFormat f;
    PCX_TRY(qformat_from_api(q, &f));
    h->qf = f;
    h->dirty = true;      // the Q-format taps are quantised again before the next call
    return PCX_OK;
}
int pcx_fir_get_geometry(const pcx_fir *h, size_t *K, size_t *input_require)
{
    PCX_CHECK_ARG(h, "null handle");
    if (K) *K = h->K;
    if (input_require) *input_require = h->inputRequire;
    return PCX_OK;
}
int pcx_fir_last_algo(const pcx_fir *h) { return h ? h->last_algo : PCX_ERR_ARG; }
int pcx_fir_get_last_plan(const pcx_fir *h, int *plan)
{
    PCX_CHECK_ARG(h && plan, "null argument");
    *plan = h->last_plan;
    return PCX_OK;
}
int pcx_fir_set_slots(pcx_fir *h, unsigned slots)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(slots >= 128 && slots <= 1024 && slots % 128 == 0, "pcx_fir_set_slots: %u is not a multiple of 128 in 128..1024", slots);
    h->slots = slots;
    return PCX_OK;
}

static size_t fir_elem_bytes(const pcx_fir *h) { return (size_t)scalar_bytes(h->scalar) * (h->cplx ? 2 : 1); }

// N of FIRFilter.cpp:278
static size_t fir_iterations(const pcx_fir *h, size_t in_elems, size_t out_cap)
{
    if (in_elems < h->K - 1) return 0;
    const size_t a = (in_elems - (h->K - 1)) / h->M, b = out_cap / h->L;
    return std::min(a, b) * h->M;
}

static int fir_process_dev_impl(pcx_fir *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                size_t *consumed, size_t *produced, void *stream, const void *gate_word, unsigned gate_value, int *gated);

// Iterations a call may be cut at without changing any output: the block payload of the plain overlap-save plan (complex_float32,
// M = L = 1, 4096-sample blocks: block b of a call computes outputs [b S, (b + 1) S), S = 4096 - (K - 1 rounded up to 16)) where that
// plan serves the handle; the time-domain kernels and the exact integer pipelines compute every output by itself, any multiple of
// M will do (a generous one: chunks stay whole tiles).  Other float plans (long taps, resamplers) are cut at multiples of M * 4096:
// their outputs stay within the 1e-5 of the oracle either way, but are not bit-identical to an uncut call's.  (The partitioned
// long-tap plan computes block b from windows b, b - 1, ... alone -- whichever workgroup's run it falls into, so a call returns the
// same bits on any grid -- but the first blocks of a CUT call see zeros where the uncut call's windows hold samples that meet no
// tap: equal in exact arithmetic, not in the transform's rounding.)
static size_t fir_chunk_quantum(const pcx_fir *h)
{
    if (h->plan.ols_plan == PCX_FIR_PLAN_CF32_OLS4096) return 4096 - (h->K - 1 + 15) / 16 * 16;
    return h->M * 4096;
}

int pcx_fir_process_dev(pcx_fir *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                        size_t *consumed, size_t *produced, void *stream)
{
    PCX_TRACE();
    return fir_process_dev_impl(h, in_dev, in_elems, out_dev, out_cap, consumed, produced, stream, nullptr, 0, nullptr);
}
int pcx_fir_process_dev_gated(pcx_fir *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                              size_t *consumed, size_t *produced, const void *gate_dev, unsigned gate_value, void *stream, int *gated)
{
    PCX_TRACE();
    PCX_CHECK_ARG(gate_dev && gated, "null gate");
    return fir_process_dev_impl(h, in_dev, in_elems, out_dev, out_cap, consumed, produced, stream, gate_dev, gate_value, gated);
}
int pcx_gate_signal_dev(void *gate_dev, unsigned value, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(gate_dev, "null gate");
    // (diagnostic library only: the word written by the command processor instead of a one-thread kernel -- a kernel needs a slot, and beside
    // a launch that fills the device it gets one only when a workgroup of that launch exits; profiles/r04/gate_write_value.txt)
    if (PCX_ENV_SET("PCX_GATE_WRITE_VALUE")) {
        PCX_HIP(hipStreamWriteValue32(as_stream(stream), gate_dev, value, 0));
        return PCX_OK;
    }
    return launch_gate_signal(gate_dev, value, as_stream(stream));
}

static int fir_process_dev_impl(pcx_fir *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                size_t *consumed, size_t *produced, void *stream, const void *gate_word, unsigned gate_value, int *gated)
{
    PCX_CHECK_ARG(h && consumed && produced, "null argument");
    if (gated) *gated = 0;
    DeviceScope dev_scope(h->cx.device);
    *consumed = 0; *produced = 0;
    const size_t N = fir_iterations(h, in_elems, out_cap);
    if (N == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    PCX_TRY(fir_sync_tables(h));
    const size_t n_out = (N / h->M) * h->L;
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const FirPlan &p = h->plan;
    const FirChoice ch = fir_resolve(p, h->algo);
    if (ch.refused) {
        set_error("fir: OLS_FFT needs complex_float32 or float32 and K<=8193 (interpolating: L<=64 rows) or complex_float64 / complex_int16 / complex_int8 with M=L=1, 2<=K<=4097");
        return PCX_ERR_UNSUPPORTED;
    }
    const int algo = ch.algo;
    int rc;
    // only the samples the N iterations touch: N + K-1
    const size_t used_in = N + h->K - 1;
    const QShift qs = q_shift(h->qf, h->scalar);      // integer element types: fromQ<OutType> of FIRFilter.cpp:300 under the handle's reading
    if (gate_word) {
        // a gated call: only the plain complex_float32 M = L = 1 plan on 4096-sample blocks has the gate (and only its dealt launch,
        // launch_fir_cf32_ols4096 decides).  Anything else: *gated stays 0, nothing has been queued, the caller orders the halo itself.
        // (The one plan that is accepted is named, rather than the others excluded: a plan added later has no gate until it says so.)
        if (ch.plan != PCX_FIR_PLAN_CF32_OLS4096) return PCX_OK;
        rc = launch_fir_cf32_ols4096(in_dev, used_in, out_dev, n_out, h->Hspec.p, h->K, h->tw4096.p, h->sched.p, st, gate_word, gate_value, gated, h->slots);
        if (rc != PCX_OK || !*gated) return rc;
        h->last_algo = algo;
        h->last_plan = PCX_FIR_PLAN_CF32_OLS4096_GATED;
        *consumed = N;
        *produced = n_out;
        return PCX_OK;
    }
    // interpolation through polyphase ROWS: every row filtered at the input rate into a contiguous workspace row, then one
    // interleaving pass.  Long calls go in batches of iterations so that the workspace stays at kRowsWorkspaceCap bytes
    // whatever the call (it would be a second copy of the output otherwise).
    auto rows_path = [&](size_t eb, size_t Mdec, auto &&row) -> int {
        size_t nb_max = kRowsWorkspaceCap / (h->L * eb) / Mdec * Mdec;     // whole output samples per batch
        if (nb_max < Mdec) nb_max = Mdec;
        PCX_TRY(h->wsRows.ensure((N < nb_max ? N : nb_max) * h->L * eb));
        for (size_t i0 = 0; i0 < N; i0 += nb_max) {
            const size_t nb = N - i0 < nb_max ? N - i0 : nb_max;
            const char *in_b = static_cast<const char *>(in_dev) + i0 * eb;   // the rows run at M = 1: one input sample per iteration
            for (size_t jr = 0; jr < h->L; jr++) PCX_TRY(row(in_b, nb, static_cast<char *>(h->wsRows.p) + jr * nb * eb, jr));
            PCX_TRY(launch_interleave_rows(h->wsRows.p, static_cast<char *>(out_dev) + i0 * h->L / Mdec * eb, nb, h->L, eb, Mdec, st));
        }
        return PCX_OK;
    };
    const auto row_of = [](const DevBuf &b, size_t jr, size_t bytes) { return static_cast<const char *>(b.p) + jr * bytes; };
    const int io64 = h->scalar == PCX_F64 ? 0 : h->scalar == PCX_I16 ? 1 : 2;     // element type of the double pipeline's loads and stores
    const FirGeom g{h->L, h->M, h->K, static_cast<const uint32_t *>(h->rowLen.p), h->rowTaps.p};
    switch (ch.plan) {
    case PCX_FIR_PLAN_F32_OLS4096_ROWS:
        rc = rows_path(4, h->M, [&](const void *in_b, size_t nb, void *dst, size_t jr) {
            return launch_fir_f32_ols4096(in_b, nb + h->K - 1, dst, nb, row_of(h->HspecRows, jr, 2 * 4096 * sizeof(float)), h->K, h->tw4096.p, h->sched.p, st);
        });
        break;
    case PCX_FIR_PLAN_REAL64_OLS_ROWS:
        rc = rows_path(fir_elem_bytes(h), h->M, [&](const void *in_b, size_t nb, void *dst, size_t jr) {
            return launch_fir_real_ols(in_b, nb + h->K - 1, dst, nb, row_of(h->HrowsD, jr, 2 * 4096 * sizeof(double)), h->K, p.log2n, h->tw4096.p, io64, 1, qs, st);
        });
        break;
    case PCX_FIR_PLAN_CF64_OLS_ROWS:
        rc = rows_path(fir_elem_bytes(h), h->M, [&](const void *in_b, size_t nb, void *dst, size_t jr) {
            return launch_fir_cf64_ols(in_b, nb + h->K - 1, dst, nb, row_of(h->HrowsD, jr, 2 * 4096 * sizeof(double)), h->K, p.log2n, h->tw4096.p, io64, 1, qs, st);
        });
        break;
    case PCX_FIR_PLAN_REAL64_OLS:
        rc = launch_fir_real_ols(in_dev, used_in, out_dev, N, h->Hspec.p, h->K, p.log2n, h->tw4096.p, io64, h->M, qs, st, h->sched.p);
        break;
    case PCX_FIR_PLAN_CF64_OLS:
        rc = launch_fir_cf64_ols(in_dev, used_in, out_dev, N, h->Hspec.p, h->K, p.log2n, h->tw4096.p, io64, h->M, qs, st, h->sched.p);
        break;
    case PCX_FIR_PLAN_UPOLS_ROWS:
        rc = rows_path(fir_elem_bytes(h), h->M, [&](const void *in_b, size_t nb, void *dst, size_t jr) {
            return launch_fir_cf32_upols(in_b, nb + h->K - 1, dst, nb, row_of(h->HspecRows, jr, fir_upols_table_bytes(p.parts)), h->K, p.parts, h->tw4096.p, st,
                                         !h->cplx, 1);
        });
        break;
    case PCX_FIR_PLAN_UPOLS_DECIM:
        rc = launch_fir_cf32_upols(in_dev, used_in, out_dev, N, h->Hspec.p, h->K, p.parts, h->tw4096.p, st, !h->cplx, h->M);
        break;
    case PCX_FIR_PLAN_F32_UPOLS:
        rc = launch_fir_cf32_upols(in_dev, used_in, out_dev, n_out, h->Hspec.p, h->K, p.parts, h->tw4096.p, st, true);
        break;
    case PCX_FIR_PLAN_F32_OLS4096:
        rc = launch_fir_f32_ols4096(in_dev, used_in, out_dev, n_out, h->Hspec.p, h->K, h->tw4096.p, h->sched.p, st);
        break;
    case PCX_FIR_PLAN_CF32_INTERP:
        rc = launch_fir_cf32_ols4096_interp(in_dev, used_in, out_dev, N, h->Hdecim.p, h->K, h->L, h->tw4096.p, h->sched.p, st);
        break;
    case PCX_FIR_PLAN_CF32_DECIM:
        rc = launch_fir_cf32_ols4096_decim(in_dev, used_in, out_dev, N, h->Hdecim.p, h->K, h->M, h->tw4096.p, h->sched.p, st);
        break;
    case PCX_FIR_PLAN_CF32_OLS4096_ROWS:
        rc = rows_path(8, 1, [&](const void *in_b, size_t nb, void *dst, size_t jr) {
            return launch_fir_cf32_ols4096(in_b, nb + h->K - 1, dst, nb, row_of(h->HspecRows, jr, 2 * 4096 * sizeof(float)), h->K, h->tw4096.p, h->sched.p, st);
        });
        break;
    case PCX_FIR_PLAN_CF32_POLY:
        rc = launch_fir_cf32_ols4096_poly(in_dev, used_in, out_dev, N, h->HspecRows.p, h->K, h->L, h->M, h->tw4096.p, st);
        break;
    case PCX_FIR_PLAN_CF32_UPOLS:
        rc = launch_fir_cf32_upols(in_dev, used_in, out_dev, n_out, h->Hspec.p, h->K, p.parts, h->tw4096.p, st);
        break;
    case PCX_FIR_PLAN_CF32_OLS4096:
        rc = launch_fir_cf32_ols4096(in_dev, used_in, out_dev, n_out, h->Hspec.p, h->K, h->tw4096.p, h->sched.p, st, nullptr, 0, nullptr, h->slots, h->lead_valid);
        break;
    case PCX_FIR_PLAN_CF32_DIRECT_TILE:
        rc = launch_fir_cf32_direct(in_dev, used_in, out_dev, n_out, h->tapsRev.p, h->K, h->Kp, st);
        break;
    case PCX_FIR_PLAN_DOT2:
        rc = launch_fir_ci16_dot2(in_dev, out_dev, n_out, h->K, h->tapsP.p, h->scalar == PCX_I8, qs, st);
        break;
    case PCX_FIR_PLAN_SLIDE:
        rc = launch_fir_slide(h->scalar, h->cplx, h->ctaps, algo == PCX_FIR_EXACT, h->taps24, g, in_dev, out_dev, n_out, qs, st);
        break;
    default:   // PCX_FIR_PLAN_GENERIC
        rc = launch_fir_generic(h->scalar, h->cplx, h->ctaps, algo == PCX_FIR_EXACT, g, in_dev, out_dev, n_out, qs, st);
        break;
    }
    if (rc != PCX_OK) return rc;
    h->last_algo = algo;
    h->last_plan = ch.plan;
    *consumed = N;
    *produced = n_out;
    return PCX_OK;
}

int pcx_fir_process(pcx_fir *h, const void *in, size_t in_elems, void *out, size_t out_cap, size_t *consumed, size_t *produced)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h && consumed && produced, "null argument");
    DeviceScope dev_scope(h->cx.device);
    *consumed = 0; *produced = 0;
    const size_t N = fir_iterations(h, in_elems, out_cap);
    if (N == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    const size_t esz = fir_elem_bytes(h), used_in = N + h->K - 1, n_out = (N / h->M) * h->L;
    // page-locked buffers (a pinned BufferManager's slabs): the kernels run on them in place; pageable ones are staged.
    // Everything goes through the handle's own stream.
    hipStream_t st;
    PCX_TRY(ctx_own_stream(h->cx, &st));
    PCX_TRY(fir_sync_tables(h));        // (tables first: nothing of the control plane between the transfers queued below)
    const void *din; void *dout; bool staged;
    if (n_out * esz >= drain_from() && host_page_locked(out)) {
        // the drained output (above): chunk by chunk into a device workspace, the copy engine behind.  A chunk is a whole number of
        // the plan's blocks where the plan has blocks (so that every output is computed exactly as by one call over everything --
        // the overlap-save kernels round differently at other block boundaries; lead_valid makes a chunk's first block a full
        // one), and of M iterations always
        const int nch = drain_chunks(n_out * esz);
        const size_t q = fir_chunk_quantum(h);
        size_t Nc = ((N + nch - 1) / nch + q - 1) / q * q;
        PCX_TRY(h->wsOut.dev.ensure(n_out * esz));
        PCX_TRY(drain_setup(h->cx, nch));
        if (!device_alias(in)) { PCX_TRY(h->wsIn.dev.ensure(used_in * esz)); PCX_TRY(h->wsIn.pin.ensure(used_in * esz)); }
        PCX_TRY(stage_in(in, used_in * esz, h->wsIn, st, &din));
        size_t done = 0;
        for (int c = 0; c < nch && done < N; c++) {
            const size_t n = N - done < Nc ? N - done : Nc, o0 = done / h->M * h->L, no = n / h->M * h->L;
            size_t cc = 0, pp = 0;
            h->lead_valid = done;
            const int rc = pcx_fir_process_dev(h, static_cast<const char *>(din) + done * esz, n + h->K - 1, static_cast<char *>(h->wsOut.dev.p) + o0 * esz, no,
                                               &cc, &pp, st);
            h->lead_valid = 0;
            PCX_TRY(rc);
            if (cc != n || pp != no) { set_error("fir: a chunk of the drained call came back short (%zu of %zu iterations)", cc, n); return PCX_ERR_STATE; }
            PCX_TRY(drain_chunk(h->cx, c, st, static_cast<char *>(out) + o0 * esz, static_cast<const char *>(h->wsOut.dev.p) + o0 * esz, no * esz));
            done += n;
        }
        PCX_TRY(drain_finish(h->cx, st));
        *consumed = N;
        *produced = n_out;
        return PCX_OK;
    }
    PCX_TRY(stage_reserve(out, n_out * esz, h->wsOut));
    PCX_TRY(stage_in(in, used_in * esz, h->wsIn, st, &din));
    PCX_TRY(stage_out_begin(out, n_out * esz, h->wsOut, &dout, &staged));
    // the kernel reads or writes the caller's page-locked memory in place: the launch shape of a link-bound call (host_grid above)
    const unsigned keep_slots = h->slots;
    int rc;
    {
        LinkBound shape(in, out);                      // (every static plan: persistent_grid / stream_grid look at it)
        if (g_link_grid) h->slots = g_link_grid;       // (the dealt plain plan: slots < 128 = that many workgroups, no dealer)
        rc = pcx_fir_process_dev(h, din, used_in, dout, n_out, consumed, produced, st);
    }
    h->slots = keep_slots;
    PCX_TRY(rc);
    return stage_out_end(out, *produced * esz, h->wsOut, staged, st);
}

/* ===================================================================== *
 *  fused Rotate -> FIR -> FreqDemod
 * ===================================================================== */
struct pcx_fmchain {
    ExecCtx cx;
    double phase = 0.0;
    bool phase_set = false;  // Rotate before setPhase: zero phasor (Rotate.cpp:60-62)
    std::vector<double> taps;
    size_t ntaps = 1;
    int ctaps = 0;
    bool dirty = true;
    size_t K = 1, Kp = 8;
    DevBuf tapsRev, Hspec, tw4096, prev;
    StageBuf wsIn, wsOut;
    DevBuf sched;   // dynamic block assignment of the fused kernel (pcx_sched.hpp), zeroed at create
    unsigned slots = 1024;
    int cur = 0;
    int algo = PCX_FIR_AUTO, last_algo = 0;
    bool have_ols = false;
    // filters longer than the fused kernels' plans (K > 2048): the FIR stage as its own launch (any K),
    // FreqDemod behind it on the same carried state
    pcx_fir *long_fir = nullptr;
    DevBuf long_y;
    ~pcx_fmchain() { delete long_fir; }
};
int pcx_fmchain_create(pcx_fmchain **out)
{
    PCX_CHECK_ARG(out, "null out");
    pcx_fmchain *h = new (std::nothrow) pcx_fmchain();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->taps.assign(1, 1.0);
    DeviceScope dev_scope(h->cx.device);
    int rc = h->prev.ensure_zeroed(64);
    if (rc == PCX_OK) rc = h->sched.ensure_zeroed(kSchedBytes);
    if (rc != PCX_OK) { delete h; return rc; }
    *out = h;
    return PCX_OK;
}
int pcx_fmchain_destroy(pcx_fmchain *h) { delete h; return PCX_OK; }
int pcx_fmchain_set_phase(pcx_fmchain *h, double phase)
{
    PCX_CHECK_ARG(h, "null handle");
    h->phase = phase; h->phase_set = true; h->dirty = true;
    return PCX_OK;
}
int pcx_fmchain_set_taps(pcx_fmchain *h, const double *taps, size_t ntaps, int complex_taps)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(ntaps > 0 && taps, "FIRFilter::setTaps(): taps cannot be empty");
    h->taps.assign(taps, taps + ntaps * (complex_taps ? 2 : 1));
    h->ntaps = ntaps; h->ctaps = complex_taps ? 1 : 0; h->dirty = true;
    return PCX_OK;
}
int pcx_fmchain_reset(pcx_fmchain *h)
{
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    // as pcx_freqdemod_reset: ordered behind the previous call and ahead of the next one
    hipStream_t st;
    PCX_TRY(ctx_state_stream(h->cx, &st));
    PCX_TRY(launch_zero_words(h->prev.p, 16, st));   // (a kernel, not hipMemsetAsync: see launch_zero_words)
    h->cur = 0;
    return PCX_OK;
}
static int fmchain_sync(pcx_fmchain *h)
{
    if (!h->dirty) return PCX_OK;
    PCX_TRY(ctx_quiesce(h->cx));   // an earlier call's kernel may still be reading the tables rewritten below
    const size_t K = h->ntaps;
    h->K = K;
    h->Kp = (K + 7) / 8 * 8;
    // Rotate's phasor folded into the taps: FIR(p*x) = (p*h) (*) x.  p is first narrowed
    // to float as floatToQ<complex<float>> does (Rotate.cpp:74), h as FIRFilter.cpp:348.
    const std::complex<double> pd = std::polar(1.0, h->phase);   // the expression of Rotate::setPhase (Rotate.cpp:74)
    const std::complex<double> p = h->phase_set ? std::complex<double>((double)(float)pd.real(), (double)(float)pd.imag())
                                                : std::complex<double>(0.0, 0.0);
    std::vector<float> rev(2 * h->Kp, 0.f);
    for (size_t m = 0; m < K; m++) {
        const size_t k = K - 1 - m;
        const std::complex<double> t = h->ctaps ? std::complex<double>((double)(float)h->taps[2 * k], (double)(float)h->taps[2 * k + 1])
                                                : std::complex<double>((double)(float)h->taps[k], 0.0);
        const std::complex<double> g = p * t;
        rev[2 * m] = (float)g.real();
        rev[2 * m + 1] = (float)g.imag();
    }
    PCX_TRY(upload(h->tapsRev, rev));
    h->have_ols = false;
    if (K <= 2048) {   // frequency-domain variant: H' = FFT(p * h) / 4096
        std::vector<std::complex<double>> g(K);
        for (size_t m = 0; m < K; m++) g[K - 1 - m] = std::complex<double>((double)rev[2 * m], (double)rev[2 * m + 1]);
        PCX_TRY(upload(h->Hspec, make_hspec4096(g)));
        PCX_TRY(upload(h->tw4096, make_tw4096()));
        h->have_ols = true;
    } else {
        // unfused long-filter path: complex taps g = p * h through the FIR handle (frequency-domain plans to
        // 8193 taps, the reference-order kernel beyond)
        if (!h->long_fir) PCX_TRY(pcx_fir_create(PCX_F32, 1, 1, &h->long_fir));
        std::vector<double> g(2 * K);
        for (size_t m = 0; m < K; m++) { g[2 * (K - 1 - m)] = (double)rev[2 * m]; g[2 * (K - 1 - m) + 1] = (double)rev[2 * m + 1]; }
        PCX_TRY(pcx_fir_set_taps(h->long_fir, g.data(), K));
    }
    h->dirty = false;
    return PCX_OK;
}
// (internal, pcx_shard.hip) upload the chain's tables now instead of at its next call
namespace pcx {
int fmchain_prepare(pcx_fmchain *h)
{
    DeviceScope dev_scope(h->cx.device);
    return fmchain_sync(h);
}
void fmchain_set_slots(pcx_fmchain *h, unsigned slots) { h->slots = slots; }
}  // namespace pcx
int pcx_fmchain_set_algo(pcx_fmchain *h, int algo)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(algo == PCX_FIR_AUTO || algo == PCX_FIR_DIRECT || algo == PCX_FIR_OLS_FFT, "fm chain: algorithm %d not available", algo);
    h->algo = algo;
    return PCX_OK;
}
int pcx_fmchain_last_algo(const pcx_fmchain *h) { return h ? h->last_algo : PCX_ERR_ARG; }
int pcx_fmchain_set_slots(pcx_fmchain *h, unsigned slots)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(slots >= 128 && slots <= 1024 && slots % 128 == 0, "pcx_fmchain_set_slots: %u is not a multiple of 128 in 128..1024", slots);
    h->slots = slots;
    return PCX_OK;
}
static int fmchain_process_dev_impl(pcx_fmchain *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                    size_t *consumed, size_t *produced, void *stream, const void *gate_word, unsigned gate_value, int *gated);
int pcx_fmchain_process_dev(pcx_fmchain *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                            size_t *consumed, size_t *produced, void *stream)
{
    PCX_TRACE();
    return fmchain_process_dev_impl(h, in_dev, in_elems, out_dev, out_cap, consumed, produced, stream, nullptr, 0, nullptr);
}
int pcx_fmchain_process_dev_gated(pcx_fmchain *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                  size_t *consumed, size_t *produced, const void *gate_dev, unsigned gate_value, void *stream, int *gated)
{
    PCX_TRACE();
    PCX_CHECK_ARG(gate_dev && gated, "null gate");
    return fmchain_process_dev_impl(h, in_dev, in_elems, out_dev, out_cap, consumed, produced, stream, gate_dev, gate_value, gated);
}
static int fmchain_process_dev_impl(pcx_fmchain *h, const void *in_dev, size_t in_elems, void *out_dev, size_t out_cap,
                                    size_t *consumed, size_t *produced, void *stream, const void *gate_word, unsigned gate_value, int *gated)
{
    PCX_CHECK_ARG(h && consumed && produced, "null argument");
    if (gated) *gated = 0;
    DeviceScope dev_scope(h->cx.device);
    *consumed = 0; *produced = 0;
    PCX_TRY(fmchain_sync(h));
    if (in_elems < h->K) return PCX_OK;
    const size_t N = std::min(in_elems - (h->K - 1), out_cap);
    if (N == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    char *base = static_cast<char *>(h->prev.p);
    PCX_TRY(ctx_enter(h->cx, as_stream(stream)));
    int algo = h->algo;
    if (gate_word && !(h->have_ols && (algo == PCX_FIR_AUTO || algo == PCX_FIR_OLS_FFT))) return PCX_OK;   // no gate but in the fused frequency-domain kernel
    if (algo == PCX_FIR_AUTO && !h->have_ols) {
        // K > 2048: two launches (FIR with the folded phasor, then FreqDemod) sharing the chain's carried state
        // (in batches: the intermediate FIR output stays at kRowsWorkspaceCap bytes whatever the call; the demodulator's state
        // walks through the batches exactly as it does through work() calls)
        const size_t nb_max = kRowsWorkspaceCap / 8;
        PCX_TRY(h->long_y.ensure((N < nb_max ? N : nb_max) * 8));
        for (size_t i0 = 0; i0 < N; i0 += nb_max) {
            const size_t nb = N - i0 < nb_max ? N - i0 : nb_max;
            size_t c2 = 0, p2 = 0;
            PCX_TRY(pcx_fir_process_dev(h->long_fir, static_cast<const float2 *>(in_dev) + i0, nb + h->K - 1, h->long_y.p, nb, &c2, &p2, stream));
            if (c2 != nb || p2 != nb) { set_error("fm chain: FIR stage produced %zu of %zu", p2, nb); return PCX_ERR_STATE; }
            PCX_TRY(launch_freqdemod(PCX_F32, h->long_y.p, static_cast<float *>(out_dev) + i0, nb, base + 32 * h->cur, base + 32 * (h->cur ^ 1),
                                     as_stream(stream)));
            h->cur ^= 1;
        }
        h->last_algo = PCX_FIR_AUTO;
        *consumed = N; *produced = N;
        return PCX_OK;
    }
    if (algo == PCX_FIR_AUTO) algo = PCX_FIR_OLS_FFT;
    if (algo == PCX_FIR_OLS_FFT) {
        if (!h->have_ols) { set_error("fm chain: OLS_FFT needs K <= 2048"); return PCX_ERR_UNSUPPORTED; }
        PCX_TRY(launch_fmchain_cf32_ols4096(in_dev, N + h->K - 1, out_dev, N, h->Hspec.p, h->K, h->tw4096.p, base + 32 * h->cur,
                                            base + 32 * (h->cur ^ 1), h->sched.p, as_stream(stream), gate_word, gate_value, gated, h->slots));
        if (gate_word && !*gated) return PCX_OK;      // a short call: the grid-stride kernel has no gate, nothing was queued
    } else {
        PCX_TRY(launch_fmchain_cf32(in_dev, N + h->K - 1, out_dev, N, h->tapsRev.p, h->K, h->Kp, base + 32 * h->cur,
                                    base + 32 * (h->cur ^ 1), as_stream(stream)));
    }
    h->last_algo = algo;
    h->cur ^= 1;
    *consumed = N; *produced = N;
    return PCX_OK;
}
int pcx_fmchain_process(pcx_fmchain *h, const void *in, size_t in_elems, void *out, size_t out_cap, size_t *consumed, size_t *produced)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h && consumed && produced, "null argument");
    DeviceScope dev_scope(h->cx.device);
    *consumed = 0; *produced = 0;
    PCX_TRY(fmchain_sync(h));
    if (in_elems < h->K) return PCX_OK;
    const size_t N = std::min(in_elems - (h->K - 1), out_cap);
    if (N == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    const size_t used = N + h->K - 1;
    return host_call(h, in, used * 8, out, N * 4, [&](const void *din, void *dout, hipStream_t st) {
        LinkBound shape(in, out);                      // (pcx_fir_process: a link-bound call's launch shape)
        const unsigned keep_slots = h->slots;
        if (g_link_grid) h->slots = g_link_grid;
        const int rc = pcx_fmchain_process_dev(h, din, used, dout, N, consumed, produced, st);
        h->slots = keep_slots;
        return rc;
    });
}
