// pcx_pre_api.hip -- the pcx_preamble handle (include/pcx.h): /comms/preamble_correlator's preamble and threshold, the plan, the
// preamble packed by bit plane and how a call is cut for preamble.hip.  The workspace of one slice is allocated and the packed
// preamble uploaded in create / set_preamble where a device can be reached (else at the first computing call); a process_dev call
// then allocates nothing on the device and walks its positions in slices, each ranking its matches behind those of the one before.
#include <vector>

#include "pcx_host.hpp"

using namespace pcx;

struct pcx_preamble {
    ExecCtx cx;
    PreShape p;
    std::vector<unsigned char> pre{1};
    bool ready = false;               // the workspace exists and tab holds this preamble
    DevBuf tab;                       // pre_table_words() packed words, then the P symbols as they are (the BYTES plan)
    DevBuf mask, counts, toff, state;
    StageBuf wsIn, wsOut;
    DevBuf res;                       // host-pointer calls: the two counts, then the indices
    PinBuf resPin;
};

namespace {
void configure(pcx_preamble *h)
{
    h->p.P = h->pre.size();
    uint32_t any = 0;
    for (const unsigned char s : h->pre) any |= s;
    h->p.active = any;
    h->p.plan = h->p.P <= pre_max_planes_len() ? PCX_PRE_PLANES : PCX_PRE_BYTES;
    h->ready = false;
}
// the workspace and the table: complete on return
int prepare(pcx_preamble *h)
{
    if (h->ready) return PCX_OK;
    const size_t slice = pre_slice(), tiles = slice / pre_tile(), words = pre_table_words(), per = words / 8;
    PCX_TRY(h->mask.ensure(slice / 8));
    PCX_TRY(h->counts.ensure(tiles * sizeof(uint32_t)));
    PCX_TRY(h->toff.ensure(tiles * sizeof(uint32_t)));
    PCX_TRY(h->state.ensure(2 * sizeof(uint64_t)));
    std::vector<unsigned char> tab(words * sizeof(uint32_t) + h->pre.size(), 0);
    if (h->p.plan == PCX_PRE_PLANES) {
        uint32_t *w = reinterpret_cast<uint32_t *>(tab.data());
        for (size_t i = 0; i < h->pre.size(); i++)
            for (int b = 0; b < 8; b++)
                if ((h->pre[i] >> b) & 1) w[b * per + i / 32] |= 1u << (i % 32);
    }
    std::copy(h->pre.begin(), h->pre.end(), tab.begin() + words * sizeof(uint32_t));
    PCX_TRY(ctx_quiesce(h->cx));          // an earlier call's kernels may still read the table
    PCX_TRY(upload(h->tab, tab));
    h->ready = true;
    return PCX_OK;
}
const uint32_t *table_words(const pcx_preamble *h) { return static_cast<const uint32_t *>(h->tab.p); }
const unsigned char *table_bytes(const pcx_preamble *h) { return static_cast<const unsigned char *>(h->tab.p) + pre_table_words() * sizeof(uint32_t); }
}  // namespace

int pcx_preamble_create(pcx_preamble **out)
{
    PCX_CHECK_ARG(out, "null out");
    pcx_preamble *h = new (std::nothrow) pcx_preamble();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    configure(h);
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_preamble_destroy(pcx_preamble *h) { delete h; return PCX_OK; }

int pcx_preamble_set_preamble(pcx_preamble *h, const unsigned char *symbols, size_t n)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(n != 0, "preamble cannot be empty");
    PCX_CHECK_ARG(symbols, "null preamble");
    h->pre.assign(symbols, symbols + n);
    configure(h);
    if (!device_reachable()) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    return prepare(h);
}
int pcx_preamble_get_preamble(const pcx_preamble *h, unsigned char *out, size_t cap, size_t *n)
{
    PCX_CHECK_ARG(h && n && (out || !cap), "null argument");
    *n = h->pre.size();
    std::copy(h->pre.begin(), h->pre.begin() + std::min(cap, h->pre.size()), out);
    return PCX_OK;
}
int pcx_preamble_set_threshold(pcx_preamble *h, unsigned threshold)
{
    PCX_CHECK_ARG(h, "null handle");
    h->p.threshold = threshold;
    return PCX_OK;
}
int pcx_preamble_get_threshold(const pcx_preamble *h, unsigned *threshold)
{
    PCX_CHECK_ARG(h && threshold, "null argument");
    *threshold = h->p.threshold;
    return PCX_OK;
}
int pcx_preamble_get_plan(const pcx_preamble *h, int *plan)
{
    PCX_CHECK_ARG(h && plan, "null argument");
    *plan = h->p.plan;
    return PCX_OK;
}
int pcx_preamble_get_geometry(size_t *tile, size_t *slice, size_t *max_planes_len)
{
    PCX_CHECK_ARG(tile && slice && max_planes_len, "null argument");
    *tile = pre_tile();
    *slice = pre_slice();
    *max_planes_len = pre_max_planes_len();
    return PCX_OK;
}

int pcx_preamble_process_dev(pcx_preamble *h, const void *in_dev, size_t n_in, void *out_dev, uint64_t *idx_dev, size_t idx_cap,
                             uint64_t *n_positions_dev, uint64_t *n_matches_dev, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(n_positions_dev && n_matches_dev, "null count");
    const size_t P = h->p.P;
    const size_t npos = n_in > P ? n_in - P : 0;
    PCX_CHECK_ARG(!npos || in_dev, "null buffer");
    PCX_CHECK_ARG(!idx_cap || idx_dev, "null index buffer");
    PCX_CHECK_ARG(!npos || !out_dev || buffers_ok(in_dev, n_in, out_dev, npos, true), "preamble correlator: out overlaps in (in place means out == in)");
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    PreWork w;
    w.mask = static_cast<uint32_t *>(h->mask.p);
    w.counts = static_cast<uint32_t *>(h->counts.p);
    w.toff = static_cast<uint32_t *>(h->toff.p);
    w.state = static_cast<uint64_t *>(h->state.p);
    if (!npos) return launch_pre_empty(w.state, n_positions_dev, n_matches_dev, st);
    const size_t slice = pre_slice();
    for (size_t off = 0; off < npos; off += slice) {
        const size_t m = std::min(slice, npos - off);
        const bool last = off + m == npos;
        PCX_TRY(launch_pre_slice(h->p, in + off, out ? out + off : nullptr, m, table_words(h), table_bytes(h), w, off, off == 0, npos,
                                 last ? n_positions_dev : nullptr, last ? n_matches_dev : nullptr, idx_dev, idx_cap, st));
    }
    return PCX_OK;
}

int pcx_preamble_process(pcx_preamble *h, const void *in, size_t n_in, void *out, uint64_t *idx, size_t idx_cap, size_t *n_positions,
                         size_t *n_matches)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(n_positions && n_matches, "null count");
    const size_t P = h->p.P;
    *n_positions = *n_matches = 0;
    if (n_in <= P) return PCX_OK;
    const size_t npos = n_in - P;
    PCX_CHECK_ARG(in, "null buffer");
    PCX_CHECK_ARG(!idx_cap || idx, "null index buffer");
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st;
    PCX_TRY(ctx_own_stream(h->cx, &st));
    PCX_TRY(prepare(h));
    const size_t head = 2 * sizeof(uint64_t);
    PCX_TRY(h->res.ensure(head + idx_cap * sizeof(uint64_t)));
    PCX_TRY(h->resPin.ensure(head));
    if (out) PCX_TRY(stage_reserve(out, npos, h->wsOut));
    const void *din; void *dout = nullptr; bool staged = false;
    PCX_TRY(stage_in(in, n_in, h->wsIn, st, &din));
    if (out) PCX_TRY(stage_out_begin(out, npos, h->wsOut, &dout, &staged));
    uint64_t *cnt = static_cast<uint64_t *>(h->res.p);
    PCX_TRY(pcx_preamble_process_dev(h, din, n_in, dout, cnt + 2, idx_cap, cnt, cnt + 1, st));
    PCX_HIP(hipMemcpyAsync(h->resPin.p, cnt, head, hipMemcpyDeviceToHost, st));
    if (out) PCX_TRY(stage_out_end(out, npos, h->wsOut, staged, st));
    PCX_HIP(hipStreamSynchronize(st));
    const uint64_t *got = static_cast<const uint64_t *>(h->resPin.p);
    const size_t nm = (size_t)got[1], take = std::min(nm, idx_cap);
    if (take) {          // nothing of the call is in flight any more: the bounce buffer may grow
        PCX_TRY(h->resPin.ensure(take * sizeof(uint64_t)));
        PCX_HIP(hipMemcpyAsync(h->resPin.p, cnt + 2, take * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        PCX_HIP(hipStreamSynchronize(st));
        std::memcpy(idx, h->resPin.p, take * sizeof(uint64_t));
    }
    *n_positions = npos;
    *n_matches = nm;
    return PCX_OK;
}

int pcx_preamble_distances_dev(pcx_preamble *h, const void *in_dev, size_t n_in, uint32_t *dist_dev, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    const size_t P = h->p.P;
    if (n_in <= P) return PCX_OK;
    const size_t npos = n_in - P;
    PCX_CHECK_ARG(in_dev && dist_dev, "null buffer");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const size_t slice = pre_slice();
    for (size_t off = 0; off < npos; off += slice)
        PCX_TRY(launch_pre_distances(h->p, static_cast<const char *>(in_dev) + off, std::min(slice, npos - off), table_words(h), table_bytes(h),
                                     dist_dev + off, st));
    return PCX_OK;
}

int pcx_preamble_distances(pcx_preamble *h, const void *in, size_t n_in, uint32_t *dist, size_t *n_positions)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(n_positions, "null count");
    const size_t P = h->p.P;
    *n_positions = 0;
    if (n_in <= P) return PCX_OK;
    const size_t npos = n_in - P, bytes = npos * sizeof(uint32_t);
    PCX_CHECK_ARG(in && dist, "null buffer");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    PCX_TRY(host_call(h, in, n_in, dist, bytes, [&](const void *din, void *dout, hipStream_t st) {
        return pcx_preamble_distances_dev(h, din, n_in, static_cast<uint32_t *>(dout), st);
    }));
    *n_positions = npos;
    return PCX_OK;
}
