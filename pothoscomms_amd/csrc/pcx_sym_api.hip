// pcx_sym_api.hip -- the pcx_mapper, pcx_slicer and pcx_diffcode handles (include/pcx.h): the maps as they were set and as symbols.hip
// reads them, the encoder's plan, the carried byte and how a call is cut.  Tables are built and uploaded in create / set_map where a
// device can be reached (else at the first computing call); a process_dev call then allocates nothing on the device and walks its
// elements in slices, the coders continuing from the device-resident byte left by the slice before.
#include <vector>

#include "pcx_host.hpp"

using namespace pcx;

namespace {
// the value 1 of a stream type (the constructors' maps: SymbolMapper.cpp:58, SymbolSlicer.cpp:64)
std::vector<unsigned char> one_element(int scalar, bool cplx)
{
    const size_t sb = (size_t)scalar_bytes(scalar);
    std::vector<unsigned char> e(sb * (cplx ? 2 : 1), 0);
    switch (scalar) {
    case PCX_F64: { const double v = 1; std::memcpy(e.data(), &v, sb); break; }
    case PCX_F32: { const float v = 1; std::memcpy(e.data(), &v, sb); break; }
    default: e[0] = 1;          // little-endian integers
    }
    return e;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- mapper
struct pcx_mapper {
    ExecCtx cx;
    int scalar = PCX_F32;
    bool cplx = false;
    size_t es = 4;                    // bytes of an element
    std::vector<unsigned char> map;   // as set, in the stream type's layout
    bool ready = false;               // tab holds this map
    DevBuf tab;                       // 256 elements: entry b = map[b & mask]
    StageBuf wsIn, wsOut;
};

static int mapper_prepare(pcx_mapper *h)
{
    if (h->ready) return PCX_OK;
    const size_t n = h->map.size() / h->es;
    const size_t mask = n >= 256 ? 255 : n - 1;         // (unsigned char)((1 << nbits) - 1), SymbolMapper.cpp:76
    std::vector<unsigned char> tab(256 * 16, 0);
    for (size_t b = 0; b < 256; b++) std::memcpy(tab.data() + b * h->es, h->map.data() + (b & mask) * h->es, h->es);
    PCX_TRY(ctx_quiesce(h->cx));          // an earlier call's kernels may still read the table
    PCX_TRY(upload(h->tab, tab));
    h->ready = true;
    return PCX_OK;
}

int pcx_mapper_create(int scalar, int is_complex, pcx_mapper **out)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(valid_scalar(scalar), "SymbolMapperFactory: unsupported type");
    pcx_mapper *h = new (std::nothrow) pcx_mapper();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->scalar = scalar;
    h->cplx = is_complex != 0;
    h->es = elem_bytes(scalar, h->cplx);
    h->map = one_element(scalar, h->cplx);
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = mapper_prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_mapper_destroy(pcx_mapper *h) { delete h; return PCX_OK; }

int pcx_mapper_set_map(pcx_mapper *h, const void *map, size_t n)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(n != 0, "Map must be nonzero size");
    PCX_CHECK_ARG((n & (n - 1)) == 0, "Map must be a power of two in length");
    PCX_CHECK_ARG(map, "null map");
    const unsigned char *m = static_cast<const unsigned char *>(map);
    h->map.assign(m, m + n * h->es);
    h->ready = false;
    if (!device_reachable()) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    return mapper_prepare(h);
}
int pcx_mapper_get_map(const pcx_mapper *h, void *out, size_t cap, size_t *n)
{
    PCX_CHECK_ARG(h && n && (out || !cap), "null argument");
    *n = h->map.size() / h->es;
    if (cap) std::memcpy(out, h->map.data(), std::min(cap, *n) * h->es);
    return PCX_OK;
}
int pcx_mapper_process_dev(pcx_mapper *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in_dev, n, out_dev, n * h->es, false), "symbol mapper: out overlaps in");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(mapper_prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    const size_t slice = sym_slice();
    for (size_t off = 0; off < n; off += slice)
        PCX_TRY(launch_sym_map(h->scalar, h->cplx, in + off, out + off * h->es, std::min(slice, n - off), h->tab.p, st));
    return PCX_OK;
}
int pcx_mapper_process(pcx_mapper *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in, n, out, n * h->es, false), "symbol mapper: out overlaps in");
    DeviceScope dev_scope(h->cx.device);
    return host_call(h, in, n, out, n * h->es,
                     [&](const void *din, void *dout, hipStream_t st) { return pcx_mapper_process_dev(h, din, dout, n, st); });
}

// ---------------------------------------------------------------------------------------------------------------- slicer
struct pcx_slicer {
    ExecCtx cx;
    int scalar = PCX_F32;
    bool cplx = false;
    size_t es = 4;
    std::vector<unsigned char> map;   // as set, in the stream type's layout
    bool ready = false;               // mapc holds this map
    DevBuf mapc;                      // the map in the promoted type (symbols.hip)
    StageBuf wsIn, wsOut;
};

static int slicer_prepare(pcx_slicer *h)
{
    if (h->ready) return PCX_OK;
    std::vector<unsigned char> conv;
    const std::vector<unsigned char> *src = &h->map;
    if (h->scalar == PCX_I8 || h->scalar == PCX_I16) {          // promoted to int, as the reference's subtraction promotes them
        const size_t words = h->map.size() / (size_t)scalar_bytes(h->scalar);
        conv.resize(words * sizeof(int32_t));
        for (size_t i = 0; i < words; i++) {
            int32_t v;
            if (h->scalar == PCX_I8) v = reinterpret_cast<const int8_t *>(h->map.data())[i];
            else { int16_t s; std::memcpy(&s, h->map.data() + 2 * i, 2); v = s; }
            std::memcpy(conv.data() + 4 * i, &v, 4);
        }
        src = &conv;
    }
    PCX_TRY(ctx_quiesce(h->cx));          // an earlier call's kernels may still read the map
    PCX_TRY(upload(h->mapc, *src));
    h->ready = true;
    return PCX_OK;
}

int pcx_slicer_create(int scalar, int is_complex, pcx_slicer **out)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(valid_scalar(scalar), "SymbolSlicerFactory: unsupported type");
    pcx_slicer *h = new (std::nothrow) pcx_slicer();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->scalar = scalar;
    h->cplx = is_complex != 0;
    h->es = elem_bytes(scalar, h->cplx);
    h->map = one_element(scalar, h->cplx);
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = slicer_prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_slicer_destroy(pcx_slicer *h) { delete h; return PCX_OK; }

int pcx_slicer_set_map(pcx_slicer *h, const void *map, size_t n)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(n != 0, "Map must be nonzero size");
    PCX_CHECK_ARG(map, "null map");
    PCX_CHECK_ARG(n <= (size_t)1 << 30, "symbol slicer: a map of %zu entries", n);
    const unsigned char *m = static_cast<const unsigned char *>(map);
    h->map.assign(m, m + n * h->es);
    h->ready = false;
    if (!device_reachable()) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    return slicer_prepare(h);
}
int pcx_slicer_get_map(const pcx_slicer *h, void *out, size_t cap, size_t *n)
{
    PCX_CHECK_ARG(h && n && (out || !cap), "null argument");
    *n = h->map.size() / h->es;
    if (cap) std::memcpy(out, h->map.data(), std::min(cap, *n) * h->es);
    return PCX_OK;
}
int pcx_slicer_get_geometry(const pcx_slicer *h, size_t *lane, size_t *group, size_t *max_onchip_map, size_t *slice)
{
    PCX_CHECK_ARG(h && lane && group && max_onchip_map && slice, "null argument");
    *lane = slicer_lane_samples(h->scalar, h->cplx);
    *group = slicer_block_samples(h->scalar, h->cplx);
    *max_onchip_map = slicer_max_onchip();
    *slice = sym_slice();
    return PCX_OK;
}
int pcx_slicer_process_dev(pcx_slicer *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in_dev, n * h->es, out_dev, n, false), "symbol slicer: out overlaps in");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(slicer_prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    const size_t slice = sym_slice(), M = h->map.size() / h->es;
    for (size_t off = 0; off < n; off += slice)
        PCX_TRY(launch_sym_slice(h->scalar, h->cplx, in + off * h->es, out + off, std::min(slice, n - off), h->mapc.p, M, st));
    return PCX_OK;
}
int pcx_slicer_process(pcx_slicer *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in, n * h->es, out, n, false), "symbol slicer: out overlaps in");
    DeviceScope dev_scope(h->cx.device);
    return host_call(h, in, n * h->es, out, n,
                     [&](const void *din, void *dout, hipStream_t st) { return pcx_slicer_process_dev(h, din, dout, n, st); });
}

// ---------------------------------------------------------------------------------------------------------------- differential coders
struct pcx_diffcode {
    ExecCtx cx;
    DiffShape p;
    bool ready = false;               // the carried byte and the workspace exist
    DevBuf state;                     // [0] the carried byte
    DevBuf tsum, tin;                 // per tile of a slice: the tile's sum, the value in front of it (decoder: the byte in front of it)
    StageBuf wsIn, wsOut;
};

// the encoder's step against (in + last) mod min(symbols, 256), over every pair of bytes
static int diff_plan(uint32_t symbols)
{
    const uint32_t m = symbols < 256 ? symbols : 256;
    for (uint32_t last = 0; last < 256; last++)
        for (uint32_t in = 0; in < 256; in++)
            if ((uint8_t)((uint32_t)(in + last + symbols) % symbols) != (uint8_t)((in + last) % m)) return PCX_DIFF_SERIAL;
    return PCX_DIFF_SCAN;
}
static int diff_prepare(pcx_diffcode *h)
{
    if (h->ready) return PCX_OK;
    const size_t tiles = sym_slice() / sym_tile();
    PCX_TRY(h->state.ensure_zeroed(4 * sizeof(uint32_t)));
    PCX_TRY(h->tsum.ensure(tiles * sizeof(uint32_t)));
    PCX_TRY(h->tin.ensure(tiles * sizeof(uint32_t)));
    h->ready = true;
    return PCX_OK;
}

int pcx_diffcode_create(int decode, pcx_diffcode **out)
{
    PCX_CHECK_ARG(out, "null out");
    pcx_diffcode *h = new (std::nothrow) pcx_diffcode();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->p.decode = decode != 0;
    h->p.symbols = 2;
    h->p.plan = h->p.decode ? PCX_DIFF_SCAN : diff_plan(2);
    if (device_reachable()) {
        DeviceScope dev_scope(h->cx.device);
        const int rc = diff_prepare(h);
        if (rc != PCX_OK) { (void)hipGetLastError(); delete h; return rc; }
    }
    *out = h;
    return PCX_OK;
}
int pcx_diffcode_destroy(pcx_diffcode *h) { delete h; return PCX_OK; }

int pcx_diffcode_set_symbols(pcx_diffcode *h, uint32_t symbols)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(symbols != 0, "symbols cannot be 0");
    h->p.symbols = symbols;
    h->p.plan = h->p.decode ? PCX_DIFF_SCAN : diff_plan(symbols);
    return PCX_OK;
}
int pcx_diffcode_get_symbols(const pcx_diffcode *h, uint32_t *symbols)
{
    PCX_CHECK_ARG(h && symbols, "null argument");
    *symbols = h->p.symbols;
    return PCX_OK;
}
int pcx_diffcode_get_plan(const pcx_diffcode *h, int *plan)
{
    PCX_CHECK_ARG(h && plan, "null argument");
    *plan = h->p.plan;
    return PCX_OK;
}
int pcx_diffcode_get_geometry(size_t *tile, size_t *slice)
{
    PCX_CHECK_ARG(tile && slice, "null argument");
    *tile = sym_tile();
    *slice = sym_slice();
    return PCX_OK;
}
int pcx_diffcode_get_state(pcx_diffcode *h, unsigned char *last)
{
    PCX_CHECK_ARG(h && last, "null argument");
    *last = 0;
    if (!h->ready) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    uint32_t w = 0;
    PCX_TRY(ctx_read_back(h->cx, &w, h->state.p, sizeof(w)));
    *last = (unsigned char)w;
    return PCX_OK;
}
int pcx_diffcode_reset(pcx_diffcode *h)
{
    PCX_CHECK_ARG(h, "null handle");
    if (!h->ready) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(ctx_quiesce(h->cx));
    return upload(h->state, std::vector<uint32_t>(4, 0));
}
int pcx_diffcode_process_dev(pcx_diffcode *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in_dev, n, out_dev, n, true), "differential coder: out overlaps in (in place means out == in)");
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(diff_prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    const size_t slice = sym_slice();
    for (size_t off = 0; off < n; off += slice)
        PCX_TRY(launch_diff_slice(h->p, in + off, out + off, std::min(slice, n - off), static_cast<uint32_t *>(h->state.p),
                                  static_cast<uint32_t *>(h->tsum.p), static_cast<uint32_t *>(h->tin.p), st));
    return PCX_OK;
}
int pcx_diffcode_process(pcx_diffcode *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(in && out, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in, n, out, n, true), "differential coder: out overlaps in (in place means out == in)");
    DeviceScope dev_scope(h->cx.device);
    return host_call(h, in, n, out, n, [&](const void *din, void *dout, hipStream_t st) { return pcx_diffcode_process_dev(h, din, dout, n, st); });
}
