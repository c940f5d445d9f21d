// pcx_dcr_api.hip -- the pcx_dcremoval handle (include/pcx.h): /comms/dc_removal's sizes, carried state and the choice between the
// fused and the staged path of dc_removal.hip.  Every device buffer is sized when the sizes are set; a process call allocates
// nothing on the device (the staged path walks a call in chunks of kChunkBytes).
#include "pcx_host.hpp"

using namespace pcx;

namespace {
constexpr size_t kChunkBytes = 32u << 20;        // staged path: samples per chunk x element bytes
constexpr int64_t kMaxAverage = int64_t(1) << 30;
int acc_bits(int scalar)
{
    switch (scalar) {
    case PCX_I64: case PCX_I32: return 64;
    case PCX_I16: return 32;
    case PCX_I8: return 16;
    }
    return 0;
}
int64_t wrap_bits(uint64_t v, int bits)
{
    if (bits >= 64) return (int64_t)v;
    const int s = 64 - bits;
    return (int64_t)(v << s) >> s;
}
}  // namespace

struct pcx_dcremoval {
    ExecCtx cx;
    DcrShape p;
    size_t elem = 0;         // bytes per stream element
    bool fused = false;
    bool ready = false;      // sizes set and every buffer allocated
    size_t chunk = 0;        // staged: samples per chunk
    DevBuf hx;               // fused: the last H input samples
    DevBuf hist;             // staged: C x D samples, stage by stage
    DevBuf b1;               // staged: C x 2 accumulators (8 bytes each)
    DevBuf tsum;             // staged: per-tile sums / offsets of one chunk
    DevBuf ybuf;             // staged: two chunks of stage outputs (C > 1)
    DevBuf tmp;              // the state shift's scratch
    StageBuf wsIn, wsOut;
};

// device buffer sizes are whole 16-byte units: the zeroing kernel clears whole words of exactly what was asked for
static size_t r16(size_t bytes) { return (bytes + 15) / 16 * 16; }

// The shape is built aside and committed only once every buffer it needs exists.  A failed allocation leaves the handle
// unconfigured (DevBuf::ensure releases the old buffer first): its process calls are refused until set_sizes succeeds.
static int dcr_configure(pcx_dcremoval *h, size_t average, size_t cascade)
{
    PCX_CHECK_ARG(average != 0, "DCRemoval::setAverageSize(): average size cannot be zero");
    PCX_CHECK_ARG(cascade != 0, "DCRemoval::setCascadeSize(): cascade size cannot be zero");
    PCX_CHECK_ARG((int64_t)average <= kMaxAverage && cascade <= 1024, "DCRemoval: sizes (%zu, %zu) beyond this port's bounds (2^30, 1024)",
                  average, cascade);
    PCX_TRY(ctx_quiesce(h->cx));
    h->ready = false;
    DcrShape p = h->p;
    p.D = (int64_t)average;
    p.C = (int)cascade;
    const int ab = acc_bits(p.scalar);
    p.dacc = ab ? wrap_bits(average, ab) : (int64_t)average;
    p.nrm = (ab && p.cplx) ? wrap_bits((uint64_t)p.dacc * (uint64_t)p.dacc, ab) : 1;
    const int64_t h_stage = (!p.cplx && p.scalar == PCX_I8) ? p.D : p.D - 1;
    p.H = h_stage * p.C;
    const bool fused = dcr_telescopes(p.scalar, p.cplx) && p.H <= dcr_fused_halo_max();
    const size_t e = h->elem;
    size_t chunk = 0;
    int rc = PCX_OK;
    if (fused) {
        rc = h->hx.ensure_zeroed(r16((size_t)p.H * e + 16));
        if (rc == PCX_OK) rc = h->tmp.ensure(r16((size_t)p.H * e + 16));
    } else {
        const size_t tile = dcr_tile();
        chunk = std::max(tile, kChunkBytes / e / tile * tile);
        rc = h->hist.ensure_zeroed(r16((size_t)p.C * (size_t)p.D * e));
        if (rc == PCX_OK) rc = h->b1.ensure_zeroed(r16((size_t)p.C * 16));
        if (rc == PCX_OK) rc = h->tsum.ensure((chunk / tile) * 16);
        // stage outputs between stages: one chunk for C = 2 (the last stage writes out), two alternating ones beyond
        if (rc == PCX_OK && p.C > 1) rc = h->ybuf.ensure((size_t)std::min(p.C - 1, 2) * chunk * e);
        if (rc == PCX_OK) rc = h->tmp.ensure(r16((size_t)p.D * e));
    }
    if (rc != PCX_OK) {
        (void)hipGetLastError();     // (a failed hipMalloc must not surface later as the error of an unrelated launch)
        return rc;
    }
    h->p = p;
    h->fused = fused;
    h->chunk = chunk;
    h->ready = true;
    return PCX_OK;
}

// zero the carried state, enqueued behind the handle's previous call and ahead of the next (a kernel: a captured reset replays)
static int dcr_zero_state(pcx_dcremoval *h, hipStream_t st)
{
    if (h->fused) return launch_zero_words(h->hx.p, h->hx.cap / 4, st);
    PCX_TRY(launch_zero_words(h->hist.p, h->hist.cap / 4, st));
    return launch_zero_words(h->b1.p, h->b1.cap / 4, st);
}
// what every call that touches the state checks first
static int dcr_usable(const pcx_dcremoval *h)
{
    if (!h->ready) {
        set_error("DCRemoval: the handle has no sizes (the last set_sizes failed)");
        return PCX_ERR_STATE;
    }
    // the reference divides by zero here (SIGFPE): refused before anything is launched
    PCX_CHECK_ARG(h->p.dacc != 0 && h->p.nrm != 0, "DCRemoval: average size %lld narrowed to the accumulator type divides by zero",
                  (long long)h->p.D);
    return PCX_OK;
}

int pcx_dcremoval_create(int scalar, int is_complex, pcx_dcremoval **out)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(valid_scalar(scalar), "DCRemovalFactory: unsupported type (scalar %d)", scalar);
    pcx_dcremoval *h = new (std::nothrow) pcx_dcremoval();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->p.scalar = scalar;
    h->p.cplx = is_complex != 0;
    h->elem = elem_bytes(scalar, h->p.cplx);
    DeviceScope dev_scope(h->cx.device);
    const int rc = dcr_configure(h, 512, 2);        // DCRemoval.cpp's initial state
    if (rc != PCX_OK) { delete h; return rc; }
    *out = h;
    return PCX_OK;
}
int pcx_dcremoval_destroy(pcx_dcremoval *h) { delete h; return PCX_OK; }
int pcx_dcremoval_set_sizes(pcx_dcremoval *h, size_t average_size, size_t cascade_size)
{
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    return dcr_configure(h, average_size, cascade_size);
}
int pcx_dcremoval_get_sizes(const pcx_dcremoval *h, size_t *average_size, size_t *cascade_size)
{
    PCX_CHECK_ARG(h && average_size && cascade_size, "null argument");
    *average_size = (size_t)h->p.D;
    *cascade_size = (size_t)h->p.C;
    return PCX_OK;
}
int pcx_dcremoval_reset(pcx_dcremoval *h)
{
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    if (!h->ready) { set_error("DCRemoval::activate(): the handle has no sizes (the last set_sizes failed)"); return PCX_ERR_STATE; }
    hipStream_t st;
    PCX_TRY(ctx_state_stream(h->cx, &st));
    return dcr_zero_state(h, st);
}
int pcx_dcremoval_process_dev(pcx_dcremoval *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(dcr_usable(h));
    const DcrShape &p = h->p;
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const size_t e = h->elem;
    if (h->fused) {
        PCX_TRY(launch_dcr_fused(p, in_dev, out_dev, n, h->hx.p, st));
        return launch_dcr_shift(h->hx.p, in_dev, n * e, (size_t)p.H * e, h->tmp.p, st);
    }
    const size_t De = (size_t)p.D * e;
    char *hist = static_cast<char *>(h->hist.p);
    char *b1 = static_cast<char *>(h->b1.p);
    char *ybuf = static_cast<char *>(h->ybuf.p);
    for (size_t off = 0; off < n; off += h->chunk) {
        const size_t m = std::min(h->chunk, n - off);
        const char *x = static_cast<const char *>(in_dev) + off * e;
        char *o = static_cast<char *>(out_dev) + off * e;
        const char *u = x;
        for (int c = 0; c < p.C; c++) {
            const bool last = c == p.C - 1;
            char *y = last ? o : ybuf + (size_t)(c & 1) * h->chunk * e;
            PCX_TRY(launch_dcr_stage(p, u, m, hist + (size_t)c * De, h->tsum.p, b1 + 16 * c, y, x, hist, last, st));
            // stage c's history moves past this chunk once its apply has read it (stage 0's: after the last stage read x's front)
            if (c > 0) PCX_TRY(launch_dcr_shift(hist + (size_t)c * De, u, m * e, De, h->tmp.p, st));
            u = y;
        }
        PCX_TRY(launch_dcr_shift(hist, x, m * e, De, h->tmp.p, st));
    }
    return PCX_OK;
}
int pcx_dcremoval_process(pcx_dcremoval *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(dcr_usable(h));
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    const size_t bytes = n * h->elem;
    return host_call(h, in, bytes, out, bytes, [&](const void *din, void *dout, hipStream_t st) { return pcx_dcremoval_process_dev(h, din, dout, n, st); });
}
