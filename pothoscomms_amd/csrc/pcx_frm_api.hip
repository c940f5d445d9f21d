// pcx_frm_api.hip -- the pcx_framer handle (include/pcx.h): the preamble, header id and padding of /comms/preamble_framer and
// /comms/frame_insert, the host plan of a call (frame_plan.hpp) and how its table reaches splice.hip.  The sync word (every preamble
// symbol repeated symbol_width times) is uploaded in set_preamble where a device can be reached (else at the first computing call).
// A call's table -- the segments in bytes, then the words of header bits -- goes through one of two slots, each a page-locked buffer
// and a device buffer with an event behind the kernel that reads them: a call waits (on the host) only for the call before the
// previous one.  A call is therefore not something to capture into a graph.
#include <vector>

#include "frame_plan.hpp"
#include "pcx_host.hpp"

using namespace pcx;

namespace {
struct TableSlot {
    PinBuf pin;
    DevBuf dev;
    hipEvent_t ev = nullptr;
    bool pending = false;
    ~TableSlot() { if (ev) (void)hipEventDestroy(ev); }
};
}  // namespace

struct pcx_framer {
    ExecCtx cx;
    int scalar = PCX_U8;
    bool cplx = false;
    size_t es = 1;
    std::vector<unsigned char> pre{1};      // count elements
    size_t width = 1;
    frm::Settings s;
    bool ready = false;                     // pool holds the sync word
    DevBuf pool;
    TableSlot slot[2];
    int next = 0;
    StageBuf wsIn, wsOut;
};

namespace {
// the longest sync word: 256 MiB
constexpr size_t kMaxPoolBytes = (size_t)256 << 20;

bool frm_type(int scalar, int cplx) { return (scalar == PCX_U8 && !cplx) || ((scalar == PCX_F32 || scalar == PCX_F64) && cplx); }

int prepare(pcx_framer *h)
{
    if (h->ready) return PCX_OK;
    const size_t count = h->pre.size() / h->es;
    std::vector<unsigned char> word(count * h->width * h->es);
    for (size_t i = 0; i < count; i++)
        for (size_t j = 0; j < h->width; j++) std::memcpy(&word[(i * h->width + j) * h->es], &h->pre[i * h->es], h->es);
    PCX_TRY(ctx_quiesce(h->cx));          // an earlier call's kernel may still read the sync word
    PCX_TRY(upload(h->pool, word));
    h->ready = true;
    return PCX_OK;
}

int make_plan(const pcx_framer *h, size_t n_in, size_t out_cap, const pcx_frame_event *events, size_t n_events, frm::Plan *p)
{
    static_assert(sizeof(pcx_frame_event) == sizeof(frm::Event) && sizeof(pcx_frame_segment) == sizeof(frm::Segment), "the plan's structs are the ABI's");
    for (size_t i = 0; i < n_events; i++)
        if (events[i].kind > PCX_FRAME_END) { set_error("framer: event %zu has kind %u", i, events[i].kind); return PCX_ERR_ARG; }
    *p = frm::plan(h->s, n_in, out_cap, reinterpret_cast<const frm::Event *>(events), n_events);
    if (!p->error.empty()) { set_error("%s", p->error.c_str()); return PCX_ERR_ARG; }
    return PCX_OK;
}
void report(const frm::Plan &p, pcx_frame_plan *plan, unsigned char *used, uint64_t *insert_at, uint64_t *shift)
{
    plan->consumed = p.consumed;
    plan->used_events = p.used_events;
    plan->out_len = p.out_len;
    plan->n_segments = p.segs.size();
    plan->n_headers = p.headers.size();
    plan->cut = p.cut ? 1 : 0;
    if (used) std::copy(p.used.begin(), p.used.end(), used);
    if (insert_at) std::copy(p.insert_at.begin(), p.insert_at.end(), insert_at);
    if (shift) std::copy(p.shift.begin(), p.shift.end(), shift);
}
// the checks every form of a call makes before anything else, in this order
#define FRM_CHECK_CALL(h, in, n_in, events, n_events, out, out_cap, plan)                                               \
    PCX_CHECK_ARG(h, "null handle");                                                                                    \
    PCX_CHECK_ARG(plan, "null plan");                                                                                   \
    PCX_CHECK_ARG(!(n_events) || (events), "null events");                                                              \
    PCX_CHECK_ARG(!(n_in) || (in), "null buffer");                                                                      \
    PCX_CHECK_ARG(!(out_cap) || (out), "null buffer");                                                                  \
    PCX_CHECK_ARG((n_in) <= SIZE_MAX / 16 && (out_cap) <= SIZE_MAX / 16, "framer: %zu elements in, %zu out", (size_t)(n_in), (size_t)(out_cap)); \
    PCX_CHECK_ARG(!(n_in) || !(out_cap) || buffers_ok(in, (n_in) * (h)->es, out, (out_cap) * (h)->es, false), "framer: out overlaps in")
}  // namespace

int pcx_framer_create(pcx_framer **out, int scalar, int is_complex)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(frm_type(scalar, is_complex), "FramerFactory: unsupported type (scalar %d, complex %d)", scalar, is_complex);
    pcx_framer *h = new (std::nothrow) pcx_framer();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->scalar = scalar;
    h->cplx = is_complex != 0;
    h->es = elem_bytes(scalar, h->cplx);
    h->pre.assign(h->es, 0);                 // the preamble {1} of both constructors
    if (scalar == PCX_U8) h->pre[0] = 1;
    else if (scalar == PCX_F32) { const float one = 1; std::memcpy(h->pre.data(), &one, sizeof(one)); }
    else { const double one = 1; std::memcpy(h->pre.data(), &one, sizeof(one)); }
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_framer_destroy(pcx_framer *h) { delete h; return PCX_OK; }

int pcx_framer_set_preamble(pcx_framer *h, const void *symbols, size_t count, size_t symbol_width, int with_header)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(count != 0, "preamble cannot be empty");
    PCX_CHECK_ARG(symbol_width != 0, "symbol width cannot be 0");
    PCX_CHECK_ARG(symbols, "null preamble");
    PCX_CHECK_ARG(!with_header || h->cplx, "framer: a header needs a complex stream");
    PCX_CHECK_ARG(count <= kMaxPoolBytes / h->es && symbol_width <= kMaxPoolBytes / h->es / count,
                  "framer: a sync word of %zu symbols, each %zu wide, exceeds %zu bytes", count, symbol_width, kMaxPoolBytes);
    const unsigned char *p = static_cast<const unsigned char *>(symbols);
    h->pre.assign(p, p + count * h->es);
    h->width = symbol_width;
    h->s.sync_len = count * symbol_width;
    h->s.header = with_header != 0;
    h->ready = false;
    if (!device_reachable()) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    return prepare(h);
}
int pcx_framer_get_preamble(const pcx_framer *h, void *symbols, size_t cap, size_t *count, size_t *symbol_width, int *with_header)
{
    PCX_CHECK_ARG(h && count && (symbols || !cap), "null argument");
    const size_t n = h->pre.size() / h->es;
    *count = n;
    if (symbol_width) *symbol_width = h->width;
    if (with_header) *with_header = h->s.header ? 1 : 0;
    if (cap) std::memcpy(symbols, h->pre.data(), std::min(cap, n) * h->es);
    return PCX_OK;
}
int pcx_framer_set_header_id(pcx_framer *h, unsigned char id)
{
    PCX_CHECK_ARG(h, "null handle");
    h->s.header_id = id;
    return PCX_OK;
}
int pcx_framer_get_header_id(const pcx_framer *h, unsigned char *id)
{
    PCX_CHECK_ARG(h && id, "null argument");
    *id = h->s.header_id;
    return PCX_OK;
}
int pcx_framer_set_padding(pcx_framer *h, size_t elements)
{
    PCX_CHECK_ARG(h, "null handle");
    h->s.padding = elements;
    return PCX_OK;
}
int pcx_framer_get_padding(const pcx_framer *h, size_t *elements)
{
    PCX_CHECK_ARG(h && elements, "null argument");
    *elements = (size_t)h->s.padding;
    return PCX_OK;
}
int pcx_framer_get_geometry(size_t *tile_bytes, size_t *lds_segments)
{
    PCX_CHECK_ARG(tile_bytes && lds_segments, "null argument");
    *tile_bytes = splice_tile_bytes();
    *lds_segments = splice_lds_segments();
    return PCX_OK;
}
int pcx_frame_header_bits(unsigned id, unsigned length, uint64_t *bits)
{
    PCX_CHECK_ARG(bits, "null argument");
    PCX_CHECK_ARG(id <= 0xffu && length <= 0xffffu, "header: id %u, length %u", id, length);
    *bits = frm::header_bits((uint8_t)id, (uint16_t)length);
    return PCX_OK;
}

int pcx_framer_plan(const pcx_framer *h, size_t n_in, size_t out_cap, const pcx_frame_event *events, size_t n_events, pcx_frame_plan *plan,
                    unsigned char *used, uint64_t *insert_at, uint64_t *shift, pcx_frame_segment *segs, size_t seg_cap, uint64_t *header_words,
                    size_t hdr_cap)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(plan, "null plan");
    PCX_CHECK_ARG(!n_events || events, "null events");
    PCX_CHECK_ARG((!seg_cap || segs) && (!hdr_cap || header_words), "null table");
    frm::Plan p;
    PCX_TRY(make_plan(h, n_in, out_cap, events, n_events, &p));
    report(p, plan, used, insert_at, shift);
    if (seg_cap) std::memcpy(segs, p.segs.data(), std::min(seg_cap, p.segs.size()) * sizeof(pcx_frame_segment));
    if (hdr_cap) std::memcpy(header_words, p.headers.data(), std::min(hdr_cap, p.headers.size()) * sizeof(uint64_t));
    return PCX_OK;
}

namespace {
// a plan with output on device pointers: its table through the next slot, then the kernel, on st
int run_plan(pcx_framer *h, const frm::Plan &p, const void *in_dev, void *out_dev, hipStream_t st)
{
    // the table: segments in bytes with the kind in the top bits of src, the sentinel included, then the header words
    const size_t nseg = p.segs.size() - 1, es = h->es;
    const size_t seg_bytes = (nseg + 1) * sizeof(SpliceSeg), bytes = seg_bytes + p.headers.size() * sizeof(uint64_t);
    TableSlot &t = h->slot[h->next];
    h->next ^= 1;
    if (t.pending) {                      // the call that used this slot last: its kernel has read the table once the event is reached
        PCX_HIP(hipEventSynchronize(t.ev));
        t.pending = false;
    }
    if (!t.ev) PCX_HIP(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    PCX_TRY(t.pin.ensure(bytes));
    PCX_TRY(t.dev.ensure(bytes));
    SpliceSeg *tab = static_cast<SpliceSeg *>(t.pin.p);
    for (size_t k = 0; k <= nseg; k++) {
        const frm::Segment &g = p.segs[k];
        tab[k].dst = g.dst * es;
        tab[k].src = ((uint64_t)g.kind << 62) | (g.kind == frm::SEG_HEADER ? g.src : g.src * es);
    }
    if (!p.headers.empty()) std::memcpy(static_cast<char *>(t.pin.p) + seg_bytes, p.headers.data(), p.headers.size() * sizeof(uint64_t));
    unsigned char sym[16] = {};
    std::memcpy(sym, &h->pre[h->pre.size() - es], es);
    PCX_TRY(ctx_enter(h->cx, st));
    PCX_HIP(hipMemcpyAsync(t.dev.p, t.pin.p, bytes, hipMemcpyHostToDevice, st));
    const SpliceSeg *dtab = static_cast<const SpliceSeg *>(t.dev.p);
    const uint64_t *dhdr = reinterpret_cast<const uint64_t *>(static_cast<const char *>(t.dev.p) + seg_bytes);
    PCX_TRY(launch_splice(es, in_dev, h->pool.p, dtab, nseg, dhdr, out_dev, (size_t)p.out_len * es, sym, st));
    PCX_HIP(hipEventRecord(t.ev, st));
    t.pending = true;
    return PCX_OK;
}
}  // namespace

int pcx_framer_process_dev(pcx_framer *h, const void *in_dev, size_t n_in, const pcx_frame_event *events, size_t n_events, void *out_dev, size_t out_cap,
                           pcx_frame_plan *plan, unsigned char *used, uint64_t *insert_at, uint64_t *shift, void *stream)
{
    PCX_TRACE();
    FRM_CHECK_CALL(h, in_dev, n_in, events, n_events, out_dev, out_cap, plan);
    frm::Plan p;
    PCX_TRY(make_plan(h, n_in, out_cap, events, n_events, &p));
    report(p, plan, used, insert_at, shift);
    if (!p.out_len) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    return run_plan(h, p, in_dev, out_dev, as_stream(stream));
}

int pcx_framer_process(pcx_framer *h, const void *in, size_t n_in, const pcx_frame_event *events, size_t n_events, void *out, size_t out_cap,
                       pcx_frame_plan *plan, unsigned char *used, uint64_t *insert_at, uint64_t *shift)
{
    PCX_TRACE();
    FRM_CHECK_CALL(h, in, n_in, events, n_events, out, out_cap, plan);
    // planned first: only what the call consumes and produces is staged, and the one plan runs
    frm::Plan p;
    PCX_TRY(make_plan(h, n_in, out_cap, events, n_events, &p));
    report(p, plan, used, insert_at, shift);
    if (!p.out_len) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    return host_call(h, in, (size_t)p.consumed * h->es, out, (size_t)p.out_len * h->es,
                     [&](const void *din, void *dout, hipStream_t st) { return run_plan(h, p, din, dout, st); });
}
