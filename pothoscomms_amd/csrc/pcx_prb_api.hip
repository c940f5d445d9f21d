// pcx_prb_api.hip -- the pcx_probe handle (include/pcx.h): /comms/signal_probe's mode and window, and the scratch of probe.hip's
// large-window path.  The scratch (a pair of doubles per slice, probe_max_slices() of them) is allocated in create where a device can
// be reached (else at the first computing call); a *_dev call then allocates nothing on the device.
#include "pcx_host.hpp"

using namespace pcx;

struct pcx_probe {
    ExecCtx cx;
    int scalar = PCX_F32;
    bool cplx = true;
    int mode = PCX_PROBE_VALUE;       // SignalProbe.cpp:64-67
    size_t window = 1024;
    bool ready = false;
    DevBuf part;
    StageBuf wsIn, wsOut;
};

namespace {
bool prb_scalar(int s) { return s >= PCX_F64 && s <= PCX_I8; }       // signalProbeFactory (SignalProbe.cpp:176-188): signed or floating
int prepare(pcx_probe *h)
{
    if (h->ready) return PCX_OK;
    PCX_TRY(h->part.ensure(probe_max_slices() * 2 * sizeof(double)));
    h->ready = true;
    return PCX_OK;
}
size_t windows_of(const pcx_probe *h, size_t n) { return (n + h->window - 1) / h->window; }
}  // namespace

int pcx_probe_create(pcx_probe **out, int scalar, int is_complex)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(prb_scalar(scalar), "signalProbeFactory: unsupported type (scalar %d)", scalar);
    pcx_probe *h = new (std::nothrow) pcx_probe();
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
int pcx_probe_destroy(pcx_probe *h) { delete h; return PCX_OK; }

int pcx_probe_set_mode(pcx_probe *h, int mode)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(mode == PCX_PROBE_VALUE || mode == PCX_PROBE_RMS || mode == PCX_PROBE_MEAN, "signal probe: unknown mode %d", mode);
    h->mode = mode;                   // (passed to the kernels by value: nothing in flight reads it)
    return PCX_OK;
}
int pcx_probe_get_mode(const pcx_probe *h, int *mode)
{
    PCX_CHECK_ARG(h && mode, "null argument");
    *mode = h->mode;
    return PCX_OK;
}
int pcx_probe_set_window(pcx_probe *h, size_t window)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(window != 0, "signal probe: the window cannot be 0");
    h->window = window;
    return PCX_OK;
}
int pcx_probe_get_window(const pcx_probe *h, size_t *window)
{
    PCX_CHECK_ARG(h && window, "null argument");
    *window = h->window;
    return PCX_OK;
}
int pcx_probe_get_geometry(const pcx_probe *h, size_t *tile, size_t *slice, size_t *switch_over)
{
    PCX_CHECK_ARG(h && tile && slice && switch_over, "null argument");
    *tile = probe_tile(h->scalar, h->cplx);
    *slice = probe_slice(h->scalar, h->cplx);
    *switch_over = *tile + 1;
    return PCX_OK;
}

int pcx_probe_windows_dev(pcx_probe *h, const void *in_dev, size_t n, double *values_dev, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (!n) return PCX_OK;
    PCX_CHECK_ARG(in_dev && values_dev, "null buffer");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    return launch_probe_windows(h->scalar, h->cplx, h->mode, in_dev, n, h->window, values_dev, static_cast<double *>(h->part.p), st);
}

int pcx_probe_windows(pcx_probe *h, const void *in, size_t n, double *values)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (!n) return PCX_OK;
    PCX_CHECK_ARG(in && values, "null buffer");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(prepare(h));
    return host_call(h, in, n * elem_bytes(h->scalar, h->cplx), values, windows_of(h, n) * 2 * sizeof(double), [&](const void *din, void *dout, hipStream_t st) {
        return pcx_probe_windows_dev(h, din, n, static_cast<double *>(dout), st);
    });
}

int pcx_probe_process_dev(pcx_probe *h, const void *in_dev, size_t n, double *value_re_im_dev, size_t *consumed, void *stream)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(consumed, "null count");
    PCX_CHECK_ARG(value_re_im_dev, "null value");
    PCX_CHECK_ARG(!n || in_dev, "null buffer");
    const size_t N = std::min(h->window, n);          // SignalProbe.cpp:127
    *consumed = N;
    return pcx_probe_windows_dev(h, in_dev, N, value_re_im_dev, stream);
}

int pcx_probe_process(pcx_probe *h, const void *in, size_t n, double *value_re_im, size_t *consumed)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(consumed, "null count");
    PCX_CHECK_ARG(value_re_im, "null value");
    PCX_CHECK_ARG(!n || in, "null buffer");
    const size_t N = std::min(h->window, n);
    *consumed = N;
    return pcx_probe_windows(h, in, N, value_re_im);
}
