// pcx_env_api.hip -- the pcx_envelope handle (include/pcx.h): /comms/envelope_detector's gains, lookahead and carried envelope,
// and how a call is cut for envelope.hip.  Every device buffer is allocated at create; a process call allocates nothing on the
// device and walks its outputs in slices of kSlice, each continuing from the device-resident end state of the one before.
#include <cmath>

#include "pcx_host.hpp"

using namespace pcx;

namespace {
constexpr size_t kSlice = size_t(1) << 26;     // outputs per slice
constexpr int64_t kChunkMin = 256, kChunkMax = 4096;
constexpr int64_t kWarmupMax = int64_t(1) << 16;

// W for gains g < 1: 1.5 x the steps in which a difference of one unit in the last place of a 24-bit mantissa decays below half
// of one (24 ln2 / -ln g), i.e. about 25 x the larger time constant.  Gains of 1 or more (or NaN) do not contract: no warm-up
// helps there, the resolve pass carries the stream.
int64_t auto_warmup(const EnvGains &g)
{
    const double gmax = std::max((double)g.gA, (double)g.gR);
    if (!(gmax >= 0.0 && gmax < 1.0)) return 0;
    if (gmax == 0.0) return 4;
    const double w = std::ceil(1.5 * 24.0 * std::log(2.0) / -std::log(gmax));
    return (int64_t)std::min<double>(w, (double)kWarmupMax);
}
}  // namespace

struct pcx_envelope {
    ExecCtx cx;
    EnvShape p;
    size_t elem = 0;             // bytes per input element
    float attack = 0, release = 0;
    size_t lookahead = 0;
    size_t warmup = 0;           // set_warmup's value, 0 = automatic
    DevBuf state;                // the carried envelope (one float)
    DevBuf ends;                 // per chunk of a slice: its speculative end state
    DevBuf miss;                 // per chunk of a slice: the repair found no match
    DevBuf cnt;                  // suspect chunks of the slice; chunks, repaired, resolved of the call
    StageBuf wsIn, wsOut;
};

static void env_shape(pcx_envelope *h)
{
    const int64_t W = h->warmup ? (int64_t)std::min<size_t>(h->warmup, (size_t)kWarmupMax) : auto_warmup(h->p.g);
    h->p.W = W;
    h->p.C = std::min(kChunkMax, std::max(kChunkMin, (W + 63) / 64 * 64));
}

int pcx_envelope_create(int scalar, int is_complex, pcx_envelope **out)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(valid_scalar(scalar), "EnvelopeDetectorFactory: unsupported type (scalar %d)", scalar);
    pcx_envelope *h = new (std::nothrow) pcx_envelope();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->p.scalar = scalar;
    h->p.cplx = is_complex != 0;
    h->elem = elem_bytes(scalar, h->p.cplx);
    env_shape(h);                                   // EnvelopeDetector.cpp:56-73: every gain 0, envelope 0, lookahead 0
    DeviceScope dev_scope(h->cx.device);
    const size_t chunks = kSlice / (size_t)kChunkMin;
    int rc = h->state.ensure_zeroed(16);
    if (rc == PCX_OK) rc = h->ends.ensure(chunks * sizeof(float));
    if (rc == PCX_OK) rc = h->miss.ensure(chunks);
    if (rc == PCX_OK) rc = h->cnt.ensure_zeroed(4 * sizeof(unsigned long long));
    if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    *out = h;
    return PCX_OK;
}
int pcx_envelope_destroy(pcx_envelope *h) { delete h; return PCX_OK; }

// setAttack / setRelease (EnvelopeDetector.cpp:76-99): the reference's own float expressions
int pcx_envelope_set_attack(pcx_envelope *h, float attack)
{
    PCX_CHECK_ARG(h, "null handle");
    h->attack = attack;
    h->p.g.gA = std::exp(-1 / attack);
    h->p.g.oA = 1 - h->p.g.gA;
    env_shape(h);
    return PCX_OK;
}
int pcx_envelope_get_attack(const pcx_envelope *h, float *attack)
{
    PCX_CHECK_ARG(h && attack, "null argument");
    *attack = h->attack;
    return PCX_OK;
}
int pcx_envelope_set_release(pcx_envelope *h, float release)
{
    PCX_CHECK_ARG(h, "null handle");
    h->release = release;
    h->p.g.gR = std::exp(-1 / release);
    h->p.g.oR = 1 - h->p.g.gR;
    env_shape(h);
    return PCX_OK;
}
int pcx_envelope_get_release(const pcx_envelope *h, float *release)
{
    PCX_CHECK_ARG(h && release, "null argument");
    *release = h->release;
    return PCX_OK;
}
int pcx_envelope_set_lookahead(pcx_envelope *h, size_t lookahead)
{
    PCX_CHECK_ARG(h, "null handle");
    h->lookahead = lookahead;
    return PCX_OK;
}
int pcx_envelope_get_lookahead(const pcx_envelope *h, size_t *lookahead)
{
    PCX_CHECK_ARG(h && lookahead, "null argument");
    *lookahead = h->lookahead;
    return PCX_OK;
}
int pcx_envelope_set_warmup(pcx_envelope *h, size_t warmup)
{
    PCX_CHECK_ARG(h, "null handle");
    h->warmup = warmup;
    env_shape(h);
    return PCX_OK;
}
int pcx_envelope_reset(pcx_envelope *h)
{
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st;
    PCX_TRY(ctx_state_stream(h->cx, &st));
    return launch_zero_words(h->state.p, h->state.cap / 4, st);
}
int pcx_envelope_get_state(pcx_envelope *h, float *envelope)
{
    PCX_CHECK_ARG(h && envelope, "null argument");
    DeviceScope dev_scope(h->cx.device);
    return ctx_read_back(h->cx, envelope, h->state.p, sizeof(float));
}
int pcx_envelope_get_stats(pcx_envelope *h, uint64_t *chunks, uint64_t *repaired, uint64_t *resolved)
{
    PCX_CHECK_ARG(h && chunks && repaired && resolved, "null argument");
    unsigned long long c[4];
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(ctx_read_back(h->cx, c, h->cnt.p, sizeof(c)));
    *chunks = c[1];
    *repaired = c[2];
    *resolved = c[3];
    return PCX_OK;
}

int pcx_envelope_process_dev(pcx_envelope *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    // out[i] is fed by in[i + lookahead]
    const char *in = static_cast<const char *>(in_dev) + h->lookahead * h->elem;
    float *out = static_cast<float *>(out_dev);
    for (size_t off = 0; off < n; off += kSlice) {
        const size_t m = std::min(kSlice, n - off);
        PCX_TRY(launch_envelope_slice(h->p, in + off * h->elem, out + off, m, static_cast<float *>(h->state.p),
                                      static_cast<float *>(h->ends.p), static_cast<unsigned char *>(h->miss.p),
                                      static_cast<unsigned long long *>(h->cnt.p), off == 0, st));
    }
    return PCX_OK;
}
int pcx_envelope_process(pcx_envelope *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    const size_t in_bytes = (n + h->lookahead) * h->elem, out_bytes = n * sizeof(float);
    return host_call(h, in, in_bytes, out, out_bytes,
                     [&](const void *din, void *dout, hipStream_t st) { return pcx_envelope_process_dev(h, din, dout, n, st); });
}
