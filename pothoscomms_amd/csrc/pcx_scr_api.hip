// pcx_scr_api.hip -- the pcx_scrambler handle (include/pcx.h): /comms/scrambler's and /comms/descrambler's register as GLFSR_init
// leaves it, the plan, the tables of M^(2^k) and how a call is cut for scrambler.hip.  Every device buffer is allocated at create and
// every table is built and uploaded in set_poly / set_seed; a process call allocates nothing on the device and walks its bits in
// slices, each continuing from the device-resident register left by the one before.
#include <vector>

#include "pcx_host.hpp"

using namespace pcx;

namespace {
constexpr int kPow = 27;                   // M^(2^k), k = 0 ... 26: a slice is 2^26 bits

// GLFSR_init (lfsr.h:63-83) on unsigned words: the mask is found by shifting a signed 1 << 63 right, so it is every bit from the
// polynomial's top bit upward; it is kept when polynom has no bit in 63..1
void glfsr_init(uint64_t polynom, uint64_t seed, uint64_t &polynomial, uint64_t &data, uint64_t &mask)
{
    polynomial = polynom | 1;
    data = seed;
    for (int b = 63; b >= 1; b--)
        if ((polynom >> b) & 1) {
            mask = ~uint64_t(0) << b;
            break;
        }
}

// the rows of M^(2^k), k < kPow, for the SCAN step D' = ((D << 1) ^ (bit m-1 of D ? pm : 0)): rows[k * 64 + r] has bit c set when bit c
// of D reaches bit r of M^(2^k) D
void power_rows(uint64_t pm, int m, std::vector<uint64_t> &rows)
{
    uint64_t col[64], nxt[64];
    for (int c = 0; c < 64; c++) {
        const uint64_t d = uint64_t(1) << c;
        col[c] = c < m ? (d << 1) ^ (((d >> (m - 1)) & 1) ? pm : 0) : 0;
    }
    rows.assign((size_t)kPow * 64, 0);
    for (int k = 0; k < kPow; k++) {
        for (int c = 0; c < 64; c++)
            for (int r = 0; r < 64; r++)
                if ((col[c] >> r) & 1) rows[(size_t)k * 64 + r] |= uint64_t(1) << c;
        for (int c = 0; c < 64; c++) {           // the square: column c = M (M e_c)
            uint64_t acc = 0;
            for (int j = 0; j < 64; j++)
                if ((col[c] >> j) & 1) acc ^= col[j];
            nxt[c] = acc;
        }
        for (int c = 0; c < 64; c++) col[c] = nxt[c];
    }
}
}  // namespace

struct pcx_scrambler {
    ExecCtx cx;
    ScrShape p;
    int64_t poly = 1, seed = 1;       // as given (the constructor's _polynom and _seed_value)
    DevBuf state;                     // [0] lfsr_t's data, carried; [1] the slice's end state before it is carried
    DevBuf pow;                       // two tables of kPow x 64 rows: additive / scrambler, multiplicative descrambler
    DevBuf z, tin, zl;                // per tile of a slice: zero-state end state, incoming state, the lanes' zero-state end states
    StageBuf wsIn, wsOut;
};

// GLFSR_init(poly, seed), the plan and the tables: complete on return
static int scr_configure(pcx_scrambler *h)
{
    uint64_t polynomial, data, mask = h->p.mask;
    glfsr_init((uint64_t)h->poly, (uint64_t)h->seed, polynomial, data, mask);
    int m = 0;
    while (m < 63 && !((mask >> m) & 1)) m++;
    const bool scan = mask != 0 && (polynomial >> m) == 1 && (data >> m) == 0;
    std::vector<uint64_t> tab((size_t)2 * kPow * 64, 0), rows;
    if (scan) {
        power_rows(polynomial, m, rows);
        std::copy(rows.begin(), rows.end(), tab.begin());
        power_rows(polynomial & ~uint64_t(1), m, rows);
        std::copy(rows.begin(), rows.end(), tab.begin() + (size_t)kPow * 64);
    }
    const std::vector<uint64_t> st = {data, data};
    PCX_TRY(ctx_quiesce(h->cx));          // an earlier call's kernels may still read the tables and the register
    PCX_TRY(upload(h->pow, tab));
    PCX_TRY(upload(h->state, st));
    h->p.polynomial = polynomial;
    h->p.mask = mask;
    h->p.m = m;
    h->p.plan = scan ? PCX_SCR_SCAN : PCX_SCR_SERIAL;
    return PCX_OK;
}

int pcx_scrambler_create(int descramble, pcx_scrambler **out)
{
    PCX_CHECK_ARG(out, "null out");
    pcx_scrambler *h = new (std::nothrow) pcx_scrambler();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->p.descramble = descramble != 0;
    h->p.mode = PCX_SCR_MULTIPLICATIVE;
    h->poly = 0x19;
    h->seed = 1;
    DeviceScope dev_scope(h->cx.device);
    const size_t tiles = scr_slice() / scr_tile();
    int rc = h->state.ensure(2 * sizeof(uint64_t));
    if (rc == PCX_OK) rc = h->pow.ensure((size_t)2 * kPow * 64 * sizeof(uint64_t));
    if (rc == PCX_OK) rc = h->z.ensure(tiles * sizeof(uint64_t));
    if (rc == PCX_OK) rc = h->tin.ensure(tiles * sizeof(uint64_t));
    if (rc == PCX_OK) rc = h->zl.ensure(tiles * 64 * sizeof(uint64_t));
    if (rc == PCX_OK) rc = scr_configure(h);
    if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    *out = h;
    return PCX_OK;
}
int pcx_scrambler_destroy(pcx_scrambler *h) { delete h; return PCX_OK; }

int pcx_scrambler_set_poly(pcx_scrambler *h, int64_t poly)
{
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    const int64_t keep = h->poly;
    h->poly = poly;
    const int rc = scr_configure(h);
    if (rc != PCX_OK) h->poly = keep;
    return rc;
}
int pcx_scrambler_get_poly(const pcx_scrambler *h, int64_t *poly)
{
    PCX_CHECK_ARG(h && poly, "null argument");
    *poly = h->poly;
    return PCX_OK;
}
int pcx_scrambler_set_seed(pcx_scrambler *h, int64_t seed)
{
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    const int64_t keep = h->seed;
    h->seed = seed;
    const int rc = scr_configure(h);
    if (rc != PCX_OK) h->seed = keep;
    return rc;
}
int pcx_scrambler_get_seed(const pcx_scrambler *h, int64_t *seed)
{
    PCX_CHECK_ARG(h && seed, "null argument");
    *seed = h->seed;
    return PCX_OK;
}
int pcx_scrambler_set_mode(pcx_scrambler *h, int mode)
{
    PCX_CHECK_ARG(mode == PCX_SCR_ADDITIVE || mode == PCX_SCR_MULTIPLICATIVE, "Scrambler::set_mode(): unknown mode: %d", mode);
    PCX_CHECK_ARG(h, "null handle");
    h->p.mode = mode;
    return PCX_OK;
}
int pcx_scrambler_get_mode(const pcx_scrambler *h, int *mode)
{
    PCX_CHECK_ARG(h && mode, "null argument");
    *mode = h->p.mode;
    return PCX_OK;
}
int pcx_scrambler_get_plan(const pcx_scrambler *h, int *plan)
{
    PCX_CHECK_ARG(h && plan, "null argument");
    *plan = h->p.plan;
    return PCX_OK;
}
int pcx_scrambler_get_geometry(size_t *run, size_t *tile, size_t *group, size_t *slice)
{
    PCX_CHECK_ARG(run && tile && group && slice, "null argument");
    *run = scr_run();
    *tile = scr_tile();
    *group = scr_group();
    *slice = scr_slice();
    return PCX_OK;
}
int pcx_scrambler_get_state(pcx_scrambler *h, int64_t *data, int64_t *mask)
{
    PCX_CHECK_ARG(h && data && mask, "null argument");
    DeviceScope dev_scope(h->cx.device);
    uint64_t d = 0;
    PCX_TRY(ctx_read_back(h->cx, &d, h->state.p, sizeof(d)));
    *data = (int64_t)d;
    *mask = (int64_t)h->p.mask;
    return PCX_OK;
}

int pcx_scrambler_process_dev(pcx_scrambler *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in_dev, n, out_dev, n, true), "scrambler: out overlaps in (in place means out == in)");
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    uint64_t *state = static_cast<uint64_t *>(h->state.p);
    const uint64_t *pow = static_cast<const uint64_t *>(h->pow.p);
    if (h->p.mode == PCX_SCR_MULTIPLICATIVE && h->p.descramble) pow += (size_t)kPow * 64;
    const size_t slice = scr_slice();
    for (size_t off = 0; off < n; off += slice) {
        const size_t m = std::min(slice, n - off);
        PCX_TRY(launch_scr_slice(h->p, in + off, out + off, m, state, pow, static_cast<uint64_t *>(h->z.p), static_cast<uint64_t *>(h->tin.p),
                                 static_cast<uint64_t *>(h->zl.p), st));
    }
    return PCX_OK;
}
int pcx_scrambler_process(pcx_scrambler *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    DeviceScope dev_scope(h->cx.device);
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    return host_call(h, in, n, out, n, [&](const void *din, void *dout, hipStream_t st) { return pcx_scrambler_process_dev(h, din, dout, n, st); });
}
