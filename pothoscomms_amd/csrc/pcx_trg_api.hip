// pcx_trg_api.hip -- the pcx_trigger handle (include/pcx.h): /comms/wave_trigger's level and slope, the word the search's workgroups
// meet in and the 24 bytes it leaves.  Both are allocated in create where a device can be reached (else at the first computing call);
// a *_dev call then allocates nothing on the device.  The host-pointer calls read back the hit resp. write the captured rows and
// nothing else: the searched stream stays where it lies unless it is pageable host memory, which no kernel can address.
#include <memory>

#include "pcx_host.hpp"

using namespace pcx;

struct pcx_trigger {
    ExecCtx cx;
    int scalar = PCX_F32;
    bool cplx = false;
    double level = 0.5;               // WaveTrigger.cpp:222-224
    int slope = PCX_TRIGGER_POS;
    bool ready = false;
    DevBuf best, res, starts;
    PinBuf resPin, startsPin;
    StageBuf wsIn;
    std::vector<std::unique_ptr<StageBuf>> capIn, capOut;     // host-pointer capture: a staging pair per port and direction
};

namespace {
bool trg_type(int s, bool cplx) { return (s >= PCX_F64 && s <= PCX_I8) || (!cplx && s >= PCX_U64 && s <= PCX_U8); }
int prepare(pcx_trigger *h)
{
    if (h->ready) return PCX_OK;
    PCX_TRY(h->best.ensure(sizeof(uint64_t)));
    PCX_TRY(h->res.ensure(sizeof(pcx_trigger_hit)));
    h->ready = true;
    return PCX_OK;
}
}  // namespace

static_assert(sizeof(pcx_trigger_hit) == 24, "the hit is 24 bytes");

int pcx_trigger_create(pcx_trigger **out, int scalar, int is_complex)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(trg_type(scalar, is_complex != 0), "wave trigger: unsupported type (scalar %d%s)", scalar, is_complex ? ", complex" : "");
    pcx_trigger *h = new (std::nothrow) pcx_trigger();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->scalar = scalar;
    h->cplx = is_complex != 0;
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_trigger_destroy(pcx_trigger *h) { delete h; return PCX_OK; }

int pcx_trigger_set_level(pcx_trigger *h, double level)
{
    PCX_CHECK_ARG(h, "null handle");
    h->level = level;                 // (passed to the kernels by value: nothing in flight reads it)
    return PCX_OK;
}
int pcx_trigger_get_level(const pcx_trigger *h, double *level)
{
    PCX_CHECK_ARG(h && level, "null argument");
    *level = h->level;
    return PCX_OK;
}
int pcx_trigger_set_slope(pcx_trigger *h, int slope)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(slope == PCX_TRIGGER_POS || slope == PCX_TRIGGER_NEG || slope == PCX_TRIGGER_LEVEL, "wave trigger: unknown slope %d", slope);
    h->slope = slope;
    return PCX_OK;
}
int pcx_trigger_get_slope(const pcx_trigger *h, int *slope)
{
    PCX_CHECK_ARG(h && slope, "null argument");
    *slope = h->slope;
    return PCX_OK;
}
int pcx_trigger_get_geometry(const pcx_trigger *h, size_t *tile)
{
    PCX_CHECK_ARG(h && tile, "null argument");
    *tile = trigger_tile();
    return PCX_OK;
}

double pcx_trigger_position(const pcx_trigger_hit *hit, double level)
{
    if (!hit) return 0.0;
    const float dy = hit->y1 - hit->y0;               // the reference subtracts in float (WaveTrigger.cpp:747)
    return (double)hit->i + (level - (double)hit->y0) / (double)dy;
}

int pcx_trigger_search_dev(pcx_trigger *h, const void *in_dev, size_t n, size_t from, pcx_trigger_hit *hit_dev, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(hit_dev, "null hit");
    PCX_CHECK_ARG(n < 2 || in_dev, "null buffer");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    return launch_trigger_search(h->scalar, h->cplx, in_dev, n, from, h->level, h->slope, static_cast<uint64_t *>(h->best.p), hit_dev, st);
}

int pcx_trigger_search(pcx_trigger *h, const void *in, size_t n, size_t from, pcx_trigger_hit *hit)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(hit, "null hit");
    PCX_CHECK_ARG(n < 2 || in, "null buffer");
    std::memset(hit, 0, sizeof(*hit));
    if (n < 2 || from > n - 2) return PCX_OK;         // no pair in the range: nothing to ask the device
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st;
    PCX_TRY(ctx_own_stream(h->cx, &st));
    PCX_TRY(prepare(h));
    PCX_TRY(h->resPin.ensure(sizeof(pcx_trigger_hit)));
    const void *din;
    PCX_TRY(stage_in(in, n * elem_bytes(h->scalar, h->cplx), h->wsIn, st, &din));
    PCX_TRY(pcx_trigger_search_dev(h, din, n, from, static_cast<pcx_trigger_hit *>(h->res.p), st));
    PCX_HIP(hipMemcpyAsync(h->resPin.p, h->res.p, sizeof(pcx_trigger_hit), hipMemcpyDeviceToHost, st));
    PCX_HIP(hipStreamSynchronize(st));
    std::memcpy(hit, h->resPin.p, sizeof(*hit));
    return PCX_OK;
}

int pcx_trigger_capture_dev(pcx_trigger *h, size_t nports, const void *const *ins_dev, const size_t *elem_bytes, const uint64_t *starts_dev, size_t nev, size_t W,
                            void *const *outs_dev, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(nports <= PCX_TRIGGER_MAX_PORTS, "wave trigger: %zu ports exceed %d", nports, PCX_TRIGGER_MAX_PORTS);
    if (!nports || !nev || !W) return PCX_OK;
    PCX_CHECK_ARG(ins_dev && elem_bytes && starts_dev && outs_dev, "null argument");
    for (size_t p = 0; p < nports; p++) PCX_CHECK_ARG(ins_dev[p] && outs_dev[p] && elem_bytes[p], "wave trigger: null buffer or element size on port %zu", p);
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    return launch_trigger_capture(nports, ins_dev, elem_bytes, starts_dev, nev, W, outs_dev, st);
}

int pcx_trigger_capture(pcx_trigger *h, size_t nports, const void *const *ins, const size_t *elem_bytes, const uint64_t *starts, size_t nev, size_t W,
                        void *const *outs)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(nports <= PCX_TRIGGER_MAX_PORTS, "wave trigger: %zu ports exceed %d", nports, PCX_TRIGGER_MAX_PORTS);
    if (!nports || !nev || !W) return PCX_OK;
    PCX_CHECK_ARG(ins && elem_bytes && starts && outs, "null argument");
    for (size_t p = 0; p < nports; p++) PCX_CHECK_ARG(ins[p] && outs[p] && elem_bytes[p], "wave trigger: null buffer or element size on port %zu", p);
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st;
    PCX_TRY(ctx_own_stream(h->cx, &st));
    while (h->capIn.size() < nports) h->capIn.emplace_back(new StageBuf());
    while (h->capOut.size() < nports) h->capOut.emplace_back(new StageBuf());
    // a pageable input is staged from its first captured element to its last: [lo, hi) in elements
    const uint64_t lo = *std::min_element(starts, starts + nev), hi = *std::max_element(starts, starts + nev) + W;
    PCX_TRY(h->starts.ensure(nev * sizeof(uint64_t)));
    PCX_TRY(h->startsPin.ensure(nev * sizeof(uint64_t)));
    for (size_t p = 0; p < nports; p++) PCX_TRY(stage_reserve(outs[p], nev * W * elem_bytes[p], *h->capOut[p]));
    std::memcpy(h->startsPin.p, starts, nev * sizeof(uint64_t));
    PCX_HIP(hipMemcpyAsync(h->starts.p, h->startsPin.p, nev * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    const void *din[PCX_TRIGGER_MAX_PORTS];
    void *dout[PCX_TRIGGER_MAX_PORTS];
    bool staged[PCX_TRIGGER_MAX_PORTS];
    for (size_t p = 0; p < nports; p++) {
        const size_t es = elem_bytes[p];
        if (void *a = device_alias(ins[p])) {
            din[p] = a;
        } else {
            const void *d;
            PCX_TRY(stage_in(static_cast<const char *>(ins[p]) + lo * es, (size_t)(hi - lo) * es, *h->capIn[p], st, &d));
            din[p] = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(d) - (uintptr_t)(lo * es));     // (an address only: the kernel reads from starts[e] >= lo on)
        }
        PCX_TRY(stage_out_begin(outs[p], nev * W * es, *h->capOut[p], &dout[p], &staged[p]));
    }
    PCX_TRY(pcx_trigger_capture_dev(h, nports, din, elem_bytes, static_cast<const uint64_t *>(h->starts.p), nev, W, dout, st));
    for (size_t p = 0; p < nports; p++) PCX_TRY(stage_out_end(outs[p], nev * W * elem_bytes[p], *h->capOut[p], staged[p], st));
    PCX_HIP(hipStreamSynchronize(st));
    return PCX_OK;
}
