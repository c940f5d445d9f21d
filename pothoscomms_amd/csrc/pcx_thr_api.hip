// pcx_thr_api.hip -- the pcx_threshold handle (include/pcx.h): /comms/threshold's two levels, the carried state and how a call is
// cut for threshold.hip.  The workspace of one slice is allocated in create where a device can be reached (else at the first
// computing call); a process_dev call then allocates nothing on the device and walks its elements in slices, each entered in the
// state the one before left on the device and ranking its transitions behind those of the one before.
#include "pcx_host.hpp"

using namespace pcx;

struct pcx_threshold {
    ExecCtx cx;
    ThrShape p;
    int state0 = 0;                   // the carried state while there is no workspace yet
    bool ready = false;               // the workspace exists and carry holds the state
    DevBuf mask, rec, toff, tot, carry, walk;
    StageBuf wsIn, wsOut;
    DevBuf res;                       // host-pointer calls: the three counts, then the indices
    PinBuf resPin;
};

namespace {
bool thr_scalar(int s) { return s >= PCX_F64 && s <= PCX_I8; }       // ThresholdFactory (Threshold.cpp:163-174): real, signed or floating
// a new carried state, ordered behind whatever the handle has in flight
int put_state(pcx_threshold *h, int active)
{
    PCX_TRY(ctx_quiesce(h->cx));
    const uint64_t v = active ? 1 : 0;
    return upload_bytes(h->carry, &v, sizeof(v));
}
int prepare(pcx_threshold *h)
{
    if (h->ready) return PCX_OK;
    const size_t tiles = thr_slice() / thr_tile();
    PCX_TRY(h->mask.ensure(tiles * thr_mask_words() * sizeof(uint64_t)));
    PCX_TRY(h->rec.ensure(tiles * sizeof(uint32_t)));
    PCX_TRY(h->toff.ensure(tiles * sizeof(uint32_t)));
    PCX_TRY(h->tot.ensure_zeroed(3 * sizeof(uint64_t)));
    PCX_TRY(h->walk.ensure_zeroed(sizeof(uint64_t)));
    PCX_TRY(put_state(h, h->state0));
    h->ready = true;
    return PCX_OK;
}
ThrWork work_of(const pcx_threshold *h)
{
    ThrWork w;
    w.mask = static_cast<uint64_t *>(h->mask.p);
    w.rec = static_cast<uint32_t *>(h->rec.p);
    w.toff = static_cast<uint32_t *>(h->toff.p);
    w.tot = static_cast<uint64_t *>(h->tot.p);
    w.carry = static_cast<uint64_t *>(h->carry.p);
    w.walk = static_cast<uint64_t *>(h->walk.p);
    return w;
}
}  // namespace

int pcx_threshold_create(pcx_threshold **out, int scalar)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(thr_scalar(scalar), "ThresholdFactory: unsupported type (scalar %d)", scalar);
    pcx_threshold *h = new (std::nothrow) pcx_threshold();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->p.scalar = scalar;             // both levels 0, inactive: Threshold.cpp:54-58
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_threshold_destroy(pcx_threshold *h) { delete h; return PCX_OK; }

int pcx_threshold_set_levels(pcx_threshold *h, const void *activation, const void *deactivation)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(activation && deactivation, "null level");
    const size_t es = (size_t)scalar_bytes(h->p.scalar);
    std::memcpy(h->p.act, activation, es);        // (passed to the kernels by value: nothing in flight reads them)
    std::memcpy(h->p.deact, deactivation, es);
    return PCX_OK;
}
int pcx_threshold_get_levels(const pcx_threshold *h, void *activation, void *deactivation)
{
    PCX_CHECK_ARG(h && activation && deactivation, "null argument");
    const size_t es = (size_t)scalar_bytes(h->p.scalar);
    std::memcpy(activation, h->p.act, es);
    std::memcpy(deactivation, h->p.deact, es);
    return PCX_OK;
}
int pcx_threshold_set_state(pcx_threshold *h, int active)
{
    PCX_CHECK_ARG(h, "null handle");
    h->state0 = active != 0;
    if (!h->ready) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    return put_state(h, active);
}
int pcx_threshold_reset(pcx_threshold *h) { return pcx_threshold_set_state(h, 0); }      // activate(), Threshold.cpp:111-115
int pcx_threshold_get_state(pcx_threshold *h, int *active)
{
    PCX_CHECK_ARG(h && active, "null argument");
    *active = h->state0;
    if (!h->ready) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    uint64_t v = 0;
    PCX_TRY(ctx_read_back(h->cx, &v, h->carry.p, sizeof(v)));
    *active = (int)(v & 1u);
    return PCX_OK;
}
int pcx_threshold_get_geometry(size_t *tile, size_t *slice)
{
    PCX_CHECK_ARG(tile && slice, "null argument");
    *tile = thr_tile();
    *slice = thr_slice();
    return PCX_OK;
}

int pcx_threshold_process_dev(pcx_threshold *h, const void *in_dev, size_t n, void *out_dev, uint64_t *idx_dev, size_t idx_cap, uint64_t *counts_dev,
                              void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(counts_dev, "null count");
    PCX_CHECK_ARG(!n || in_dev, "null buffer");
    PCX_CHECK_ARG(!idx_cap || idx_dev, "null index buffer");
    const size_t es = (size_t)scalar_bytes(h->p.scalar);
    PCX_CHECK_ARG(!n || !out_dev || buffers_ok(in_dev, n * es, out_dev, n * es, true), "threshold: out overlaps in (in place means out == in)");
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const ThrWork w = work_of(h);
    if (!n) return launch_thr_empty(w, counts_dev, st);
    const size_t slice = thr_slice();
    for (size_t off = 0; off < n; off += slice) {
        const size_t m = std::min(slice, n - off);
        PCX_TRY(launch_thr_slice(h->p, in + off * es, out ? out + off * es : nullptr, m, w, off, off == 0, n, off + m == n ? counts_dev : nullptr, idx_dev,
                                 idx_cap, st));
    }
    return PCX_OK;
}

int pcx_threshold_process(pcx_threshold *h, const void *in, size_t n, void *out, uint64_t *idx, size_t idx_cap, size_t *n_transitions, int *state_in)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(n_transitions && state_in, "null count");
    PCX_CHECK_ARG(!n || in, "null buffer");
    PCX_CHECK_ARG(!idx_cap || idx, "null index buffer");
    const size_t es = (size_t)scalar_bytes(h->p.scalar), bytes = n * es;
    PCX_CHECK_ARG(!n || !out || buffers_ok(in, bytes, out, bytes, true), "threshold: out overlaps in (in place means out == in)");
    *n_transitions = 0;
    if (!n) return pcx_threshold_get_state(h, state_in);
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st;
    PCX_TRY(ctx_own_stream(h->cx, &st));
    PCX_TRY(prepare(h));
    const size_t head = 3 * sizeof(uint64_t);
    PCX_TRY(h->res.ensure(head + idx_cap * sizeof(uint64_t)));
    PCX_TRY(h->resPin.ensure(head));
    if (out) PCX_TRY(stage_reserve(out, bytes, h->wsOut));
    const void *din; void *dout = nullptr; bool staged = false;
    PCX_TRY(stage_in(in, bytes, h->wsIn, st, &din));
    if (out) PCX_TRY(stage_out_begin(out, bytes, h->wsOut, &dout, &staged));
    uint64_t *cnt = static_cast<uint64_t *>(h->res.p);
    PCX_TRY(pcx_threshold_process_dev(h, din, n, dout, cnt + 3, idx_cap, cnt, st));
    PCX_HIP(hipMemcpyAsync(h->resPin.p, cnt, head, hipMemcpyDeviceToHost, st));
    if (out) PCX_TRY(stage_out_end(out, bytes, h->wsOut, staged, st));
    PCX_HIP(hipStreamSynchronize(st));
    const uint64_t *got = static_cast<const uint64_t *>(h->resPin.p);
    const size_t nt = (size_t)got[1], take = std::min(nt, idx_cap);
    const int entry = (int)got[2];
    if (take) {          // nothing of the call is in flight any more: the bounce buffer may grow
        PCX_TRY(h->resPin.ensure(take * sizeof(uint64_t)));
        PCX_HIP(hipMemcpyAsync(h->resPin.p, cnt + 3, take * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        PCX_HIP(hipStreamSynchronize(st));
        std::memcpy(idx, h->resPin.p, take * sizeof(uint64_t));
    }
    *n_transitions = nt;
    *state_in = entry;
    return PCX_OK;
}

int pcx_threshold_states_dev(pcx_threshold *h, const void *in_dev, size_t n, unsigned char *states_dev, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (!n) return PCX_OK;
    PCX_CHECK_ARG(in_dev && states_dev, "null buffer");
    const size_t es = (size_t)scalar_bytes(h->p.scalar);
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const ThrWork w = work_of(h);
    const size_t slice = thr_slice();
    for (size_t off = 0; off < n; off += slice)
        PCX_TRY(launch_thr_states(h->p, static_cast<const char *>(in_dev) + off * es, std::min(slice, n - off), w, off == 0, states_dev + off, st));
    return PCX_OK;
}

int pcx_threshold_states(pcx_threshold *h, const void *in, size_t n, unsigned char *states)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (!n) return PCX_OK;
    PCX_CHECK_ARG(in && states, "null buffer");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    return host_call(h, in, n * (size_t)scalar_bytes(h->p.scalar), states, n, [&](const void *din, void *dout, hipStream_t st) {
        return pcx_threshold_states_dev(h, din, n, static_cast<unsigned char *>(dout), st);
    });
}
