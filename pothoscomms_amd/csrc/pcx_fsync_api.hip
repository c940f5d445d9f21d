// pcx_fsync_api.hip -- the pcx_fsync handle (include/pcx.h): the settings of /comms/frame_sync, the state its work() carries from call
// to call, and the walk of one call over framesync.hip's kernels.  The state lives on the HOST: a payload call computes what it
// consumes and produces from it and only enqueues; a search call reads the tracker and the header bits back (one small copy per
// candidate frame) and decides as FrameSync.cpp:533-587 does (frame_sync_plan.hpp).  On the device the handle keeps the preamble as
// doubles, the corrPeak words of a call and the two small result records.  It keeps NO history of the stream: a frame may begin in front of
// the buffer of the call that declares it, but nothing is read there.
#include <string>
#include <vector>

#include "frame_sync_plan.hpp"
#include "pcx_host.hpp"

using namespace pcx;

struct pcx_fsync {
    ExecCtx cx;
    int scalar = PCX_F32;
    size_t es = 8;
    // settings
    std::vector<unsigned char> pre_raw;     // the preamble in the stream's type
    std::vector<double> pre;                // and as pairs of doubles
    int mode = PCX_FSYNC_RAW;
    unsigned char header_id = 0x55;
    size_t sw = 20, dw = 4;
    double thresh = 0;
    bool verbose = false;
    std::string ids[3] = {"", "frameStart", ""};
    // derived (updateSettings)
    size_t W = 80, F = 80 + PCX_FRAME_HEADER_BITS * 4, mag = 56, dur = 40;
    // carried state
    uint64_t remaining = 0, max_peak = 0, cnt = 0, reserve = 0;
    double phase = 0, phase_inc = 0;
    FsyncEst est;
    // device
    bool ready = false;
    DevBuf preDev, peaks, rec;
    StageBuf wsIn, wsOut;
};

namespace {
// the longest sync word (include/pcx.h): one lane walks it once per candidate frame, about 20 ns a sample
constexpr size_t kMaxSyncWord = (size_t)1 << 16;
// offsets of the first and of the longest piece of a search call (multiples of the metric kernel's tile)
constexpr size_t kFirstPiece = (size_t)16 << 10, kLastPiece = (size_t)4 << 20;

void update_settings(pcx_fsync *h)
{
    const size_t P = h->pre.size() / 2;
    h->W = h->sw * h->dw * P;
    h->F = h->W + (size_t)PCX_FRAME_HEADER_BITS * h->dw;
    h->mag = (size_t)((double)h->W * 0.7);
    h->dur = (size_t)((double)h->W * 0.5);
    h->ready = false;
}
FsyncShape shape_of(const pcx_fsync *h)
{
    FsyncShape s;
    const size_t P = h->pre.size() / 2;
    s.f64 = h->scalar == PCX_F64;
    s.sw = h->sw;
    s.dw = h->dw;
    s.P = P;
    s.W = h->W;
    s.F = h->F;
    s.thresh = h->thresh;
    s.abs_front = std::hypot(h->pre[0], h->pre[1]);
    s.abs_back = std::hypot(h->pre[2 * P - 2], h->pre[2 * P - 1]);
    return s;
}
int prepare(pcx_fsync *h)
{
    if (h->ready) return PCX_OK;
    PCX_TRY(ctx_quiesce(h->cx));
    PCX_TRY(upload(h->preDev, h->pre));
    PCX_TRY(h->rec.ensure(sizeof(FsyncScanOut) + sizeof(FsyncFinishOut)));
    h->ready = true;
    return PCX_OK;
}
void reset_state(pcx_fsync *h)
{
    h->remaining = h->max_peak = h->cnt = h->reserve = 0;
    h->phase = h->phase_inc = 0;
    h->est = FsyncEst();
}
void report(const pcx_fsync *h, pcx_fsync_result *r)
{
    r->reserve = h->reserve;
    r->remaining = h->remaining;
    r->phase = h->phase;
    r->phase_inc = h->phase_inc;
    r->scale = h->est.scale;
    r->delta_fc = h->est.delta_fc;
    r->phase_off = h->est.phase_off;
    r->max_peak = h->max_peak;
    r->count_since_max = h->cnt;
}
// the payload part of work() (:401-457); the caller has found remaining != 0
int payload_call(pcx_fsync *h, const void *din, size_t n, void *dout, size_t cap, pcx_fsync_result *r, hipStream_t st)
{
    const bool f64 = h->scalar == PCX_F64;
    size_t N, consumed;
    if (h->mode == PCX_FSYNC_TIMING) {
        N = std::min(std::min((size_t)h->remaining, n) / h->dw, cap);
        if (N == 0) h->reserve = h->dw;
        consumed = N * h->dw;
        PCX_TRY(launch_fsync_payload(f64, 2, din, dout, N, h->dw, h->est.scale, h->phase, h->phase_inc * (double)h->dw, st));
        h->phase += (double)N * (h->phase_inc * (double)h->dw);
    } else {
        N = std::min((size_t)h->remaining, std::min(n, cap));
        consumed = N;
        PCX_TRY(launch_fsync_payload(f64, h->mode == PCX_FSYNC_RAW ? 0 : 1, din, dout, N, h->dw, h->est.scale, h->phase, h->phase_inc, st));
        if (h->mode != PCX_FSYNC_RAW) h->phase += (double)N * h->phase_inc;
    }
    h->remaining -= consumed;
    r->consumed = consumed;
    r->produced = N;
    return PCX_OK;
}

// the search part of work() (:462-589)
int search_call(pcx_fsync *h, const void *din, size_t n, pcx_fsync_result *r, hipStream_t st)
{
    if (n < h->F) {
        h->reserve = h->F;
        return PCX_OK;
    }
    const size_t N = n - h->F + 1;
    const FsyncShape s = shape_of(h);
    const double *pre = static_cast<const double *>(h->preDev.p);
    const size_t ntiles = (N + fsync_tile() - 1) / fsync_tile();
    PCX_TRY(h->peaks.ensure((N + ntiles) * sizeof(uint32_t)));        // the corrPeak words, then a flag per tile
    uint32_t *peaks = static_cast<uint32_t *>(h->peaks.p), *flags = peaks + N;
    const uint32_t thresh = (uint32_t)std::min<size_t>(h->mag, 0xffffffffu);
    FsyncScanOut *scan_dev = static_cast<FsyncScanOut *>(h->rec.p);
    FsyncFinishOut *fin_dev = reinterpret_cast<FsyncFinishOut *>(scan_dev + 1);
    fsy::Settings fs;
    fs.dw = h->dw;
    fs.F = h->F;
    fs.mode = h->mode;
    fs.phase_id = !h->ids[PCX_FSYNC_PHASE_OFFSET].empty();
    fs.start_id = !h->ids[PCX_FSYNC_FRAME_START].empty();
    fs.end_id = !h->ids[PCX_FSYNC_FRAME_END].empty();
    // The offsets are searched in PIECES, the first of kFirstPiece offsets and every further one twice as long: a frame near the front of
    // a long buffer costs the correlation of a piece, not of the buffer, and a buffer without a frame costs a few read-backs more
    uint64_t s0 = 0;
    size_t have = 0, piece = kFirstPiece;
    for (;;) {
        if (s0 >= have) {
            if (have >= N) break;
            const size_t upto = std::min(N, have + piece);
            PCX_TRY(launch_fsync_metric(s, din, n, have, upto, pre, thresh, peaks, flags, st));
            have = upto;
            piece = std::min(piece * 2, kLastPiece);
        }
        struct { FsyncScanOut scan; FsyncFinishOut fin; } back;
        const uint32_t max0 = (uint32_t)std::min<uint64_t>(h->max_peak, 0xffffffffu);
        PCX_TRY(launch_fsync_scan(peaks, flags, s0, have, thresh, h->dur, max0, h->cnt, scan_dev, st));
        PCX_TRY(launch_fsync_finish(s, din, n, pre, h->est, scan_dev, fin_dev, st));
        PCX_TRY(ctx_read_back(h->cx, &back, scan_dev, sizeof(back)));
        h->max_peak = back.scan.max_peak;
        h->cnt = back.scan.count;
        h->est.scale = back.fin.scale;
        h->est.delta_fc = back.fin.delta_fc;
        h->est.phase_off = back.fin.phase_off;
        if (!back.scan.declared) {
            s0 = have;
            continue;
        }
        h->max_peak = 0;                  // :515
        const fsy::Header hd = back.fin.found ? fsy::decode_header(back.fin.bits) : fsy::Header();
        if (!fsy::header_accepted(hd, h->header_id)) {
            s0 = back.scan.at + 1;        // the scan goes on behind the offset that declared
            continue;
        }
        const int64_t frame_off = (int64_t)back.scan.at - (int64_t)back.scan.count;
        const fsy::Found f = fsy::frame_found(fs, frame_off, back.fin.first_bit, h->est.delta_fc, h->est.phase_off, hd.length);
        h->remaining = f.remaining;
        h->phase = f.phase;
        h->phase_inc = f.phase_inc;
        h->reserve = 0;
        r->n_labels = f.n_labels;
        for (unsigned k = 0; k < f.n_labels; k++) {
            r->labels[k].kind = f.labels[k].kind;
            r->labels[k].index = f.labels[k].index;
            r->labels[k].width = f.labels[k].width;
            r->labels[k].length = f.labels[k].length;
            r->labels[k].value = f.labels[k].value;
        }
        // (the reference would consume past its buffer where a first bit found late in the header pushes the payload offset there)
        r->consumed = std::min<uint64_t>(f.consumed, n);
        return PCX_OK;
    }
    r->consumed = N;
    return PCX_OK;
}

int run_call(pcx_fsync *h, const void *din, size_t n, void *dout, size_t cap, pcx_fsync_result *r, hipStream_t st)
{
    PCX_TRY(ctx_enter(h->cx, st));
    if (h->remaining != 0) PCX_TRY(payload_call(h, din, n, dout, cap, r, st));
    else PCX_TRY(search_call(h, din, n, r, st));
    report(h, r);
    return PCX_OK;
}

#define FSYNC_CHECK_CALL(h, in, n_in, out, out_cap, result)                                                                          \
    PCX_CHECK_ARG(h, "null handle");                                                                                              \
    PCX_CHECK_ARG(result, "null result");                                                                                         \
    PCX_CHECK_ARG(!(n_in) || (in), "null buffer");                                                                                \
    PCX_CHECK_ARG(!(out_cap) || (out), "null buffer");                                                                            \
    PCX_CHECK_ARG((n_in) <= SIZE_MAX / 32 && (out_cap) <= SIZE_MAX / 32, "frame sync: %zu elements in, %zu out", (size_t)(n_in), (size_t)(out_cap)); \
    PCX_CHECK_ARG(!(n_in) || !(out_cap) || buffers_ok(in, (n_in) * (h)->es, out, (out_cap) * (h)->es, false), "frame sync: out overlaps in"); \
    *(result) = pcx_fsync_result()
}  // namespace

int pcx_fsync_create(pcx_fsync **out, int scalar, int is_complex)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(is_complex && (scalar == PCX_F32 || scalar == PCX_F64), "FrameSyncFactory: unsupported type (scalar %d, complex %d)", scalar, is_complex);
    pcx_fsync *h = new (std::nothrow) pcx_fsync();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->scalar = scalar;
    h->es = elem_bytes(scalar, true);
    h->pre = {1.0, 0.0};
    h->pre_raw.assign(h->es, 0);
    if (scalar == PCX_F32) { const float one = 1; std::memcpy(h->pre_raw.data(), &one, sizeof(one)); }
    else { const double one = 1; std::memcpy(h->pre_raw.data(), &one, sizeof(one)); }
    h->thresh = scalar == PCX_F32 ? (double)(float)0.01 : 0.01;
    update_settings(h);
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_fsync_destroy(pcx_fsync *h) { delete h; return PCX_OK; }

int pcx_fsync_set_output_mode(pcx_fsync *h, int mode)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(mode >= PCX_FSYNC_RAW && mode <= PCX_FSYNC_DEBUG, "FrameSync::setOutputMode(%d): unknown output mode", mode);
    h->mode = mode;
    return PCX_OK;
}
int pcx_fsync_get_output_mode(const pcx_fsync *h, int *mode)
{
    PCX_CHECK_ARG(h && mode, "null argument");
    *mode = h->mode;
    return PCX_OK;
}
int pcx_fsync_set_preamble(pcx_fsync *h, const void *symbols, size_t count)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(count != 0, "FrameSync::setPreamble(): preamble cannot be empty");
    PCX_CHECK_ARG(symbols, "null preamble");
    PCX_CHECK_ARG(count <= kMaxSyncWord / h->sw / h->dw, "frame sync: a sync word of %zu symbols, each %zu wide, exceeds %zu samples", count, h->sw * h->dw,
                  kMaxSyncWord);
    const unsigned char *p = static_cast<const unsigned char *>(symbols);
    h->pre_raw.assign(p, p + count * h->es);
    h->pre.resize(2 * count);
    for (size_t k = 0; k < 2 * count; k++) {
        if (h->scalar == PCX_F32) { float v; std::memcpy(&v, p + k * sizeof(v), sizeof(v)); h->pre[k] = v; }
        else std::memcpy(&h->pre[k], p + k * sizeof(double), sizeof(double));
    }
    update_settings(h);
    return PCX_OK;
}
int pcx_fsync_get_preamble(const pcx_fsync *h, void *symbols, size_t cap, size_t *count)
{
    PCX_CHECK_ARG(h && count && (symbols || !cap), "null argument");
    const size_t n = h->pre_raw.size() / h->es;
    *count = n;
    if (cap) std::memcpy(symbols, h->pre_raw.data(), std::min(cap, n) * h->es);
    return PCX_OK;
}
int pcx_fsync_set_header_id(pcx_fsync *h, unsigned char id)
{
    PCX_CHECK_ARG(h, "null handle");
    h->header_id = id;
    return PCX_OK;
}
int pcx_fsync_get_header_id(const pcx_fsync *h, unsigned char *id)
{
    PCX_CHECK_ARG(h && id, "null argument");
    *id = h->header_id;
    return PCX_OK;
}
int pcx_fsync_set_symbol_width(pcx_fsync *h, size_t width)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(width != 0, "FrameSync::setSymbolWidth(): symbol width cannot be 0");
    PCX_CHECK_ARG(width >= 3, "FrameSync::setSymbolWidth(%zu): the envelope needs at least 3 samples per preamble symbol", width);
    PCX_CHECK_ARG(width <= kMaxSyncWord / h->dw / (h->pre.size() / 2), "frame sync: a sync word of %zu symbols, each %zu wide, exceeds %zu samples",
                  h->pre.size() / 2, width * h->dw, kMaxSyncWord);
    h->sw = width;
    update_settings(h);
    return PCX_OK;
}
int pcx_fsync_get_symbol_width(const pcx_fsync *h, size_t *width)
{
    PCX_CHECK_ARG(h && width, "null argument");
    *width = h->sw;
    return PCX_OK;
}
int pcx_fsync_set_data_width(pcx_fsync *h, size_t width)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(width >= 2, "FrameSync::setDataWidth(): data width should be at least 2 samples per symbol");
    PCX_CHECK_ARG(width <= kMaxSyncWord / h->sw / (h->pre.size() / 2), "frame sync: a sync word of %zu symbols, each %zu wide, exceeds %zu samples",
                  h->pre.size() / 2, width * h->sw, kMaxSyncWord);
    h->dw = width;
    update_settings(h);
    return PCX_OK;
}
int pcx_fsync_get_data_width(const pcx_fsync *h, size_t *width)
{
    PCX_CHECK_ARG(h && width, "null argument");
    *width = h->dw;
    return PCX_OK;
}
int pcx_fsync_set_input_threshold(pcx_fsync *h, double threshold)
{
    PCX_CHECK_ARG(h, "null handle");
    const double t = h->scalar == PCX_F32 ? (double)(float)threshold : threshold;
    PCX_CHECK_ARG(!(t < 0), "FrameSync::setInputThreshold(): threshold should be non-negative");
    h->thresh = t;
    return PCX_OK;
}
int pcx_fsync_get_input_threshold(const pcx_fsync *h, double *threshold)
{
    PCX_CHECK_ARG(h && threshold, "null argument");
    *threshold = h->thresh;
    return PCX_OK;
}
int pcx_fsync_set_verbose(pcx_fsync *h, int enable)
{
    PCX_CHECK_ARG(h, "null handle");
    h->verbose = enable != 0;
    return PCX_OK;
}
int pcx_fsync_set_label_id(pcx_fsync *h, int kind, const char *id)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(kind >= PCX_FSYNC_PHASE_OFFSET && kind <= PCX_FSYNC_FRAME_END, "frame sync: label kind %d", kind);
    h->ids[kind] = id ? id : "";
    return PCX_OK;
}
int pcx_fsync_get_label_id(const pcx_fsync *h, int kind, char *id, size_t cap, size_t *len)
{
    PCX_CHECK_ARG(h && len && (id || !cap), "null argument");
    PCX_CHECK_ARG(kind >= PCX_FSYNC_PHASE_OFFSET && kind <= PCX_FSYNC_FRAME_END, "frame sync: label kind %d", kind);
    const std::string &s = h->ids[kind];
    *len = s.size();
    if (cap) {
        const size_t m = std::min(cap - 1, s.size());
        std::memcpy(id, s.data(), m);
        id[m] = 0;
    }
    return PCX_OK;
}
int pcx_fsync_get_geometry(const pcx_fsync *h, size_t *sync_width, size_t *frame_width, size_t *corr_mag, size_t *corr_dur, size_t *tile, size_t *first_piece)
{
    PCX_CHECK_ARG(h && sync_width && frame_width && corr_mag && corr_dur && tile && first_piece, "null argument");
    *first_piece = kFirstPiece;
    *sync_width = h->W;
    *frame_width = h->F;
    *corr_mag = h->mag;
    *corr_dur = h->dur;
    *tile = fsync_tile();
    return PCX_OK;
}
int pcx_fsync_activate(pcx_fsync *h)
{
    PCX_CHECK_ARG(h, "null handle");
    reset_state(h);
    return PCX_OK;
}

int pcx_fsync_process_dev(pcx_fsync *h, const void *in_dev, size_t n_in, void *out_dev, size_t out_cap, pcx_fsync_result *result, void *stream)
{
    PCX_TRACE();
    FSYNC_CHECK_CALL(h, in_dev, n_in, out_dev, out_cap, result);
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    return run_call(h, in_dev, n_in, out_dev, out_cap, result, as_stream(stream));
}

int pcx_fsync_process(pcx_fsync *h, const void *in, size_t n_in, void *out, size_t out_cap, pcx_fsync_result *result)
{
    PCX_TRACE();
    FSYNC_CHECK_CALL(h, in, n_in, out, out_cap, result);
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    // what the call produces follows from the carried state alone: only that much of `out` is staged
    size_t produced = 0;
    if (h->remaining != 0)
        produced = h->mode == PCX_FSYNC_TIMING ? std::min(std::min((size_t)h->remaining, n_in) / h->dw, out_cap) : std::min((size_t)h->remaining, std::min(n_in, out_cap));
    return host_call(h, in, n_in * h->es, out, produced * h->es,
                     [&](const void *din, void *dout, hipStream_t st) { return run_call(h, din, n_in, dout, out_cap, result, st); });
}
