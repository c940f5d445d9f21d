// pcx_rpk_api.hip -- the pcx_repack handle (include/pcx.h): which conversion, the modulus and the bit order as they were set, the
// group the reference reserves and how a call is cut.  The handle owns nothing on the device but the staging workspaces of host_call: a
// process_dev call allocates nothing and walks its elements in slices of whole tiles, one launch each (repack.hip).
#include "pcx_host.hpp"

using namespace pcx;

struct pcx_repack {
    ExecCtx cx;
    int kind = PCX_REPACK_BITS_TO_SYMBOLS;
    unsigned mod = 1;
    bool msb = true;
    StageBuf wsIn, wsOut;
};

namespace {
// _reserveBytes (BytesToSymbols.cpp:69-76) and _reserveSyms (SymbolsToBytes.cpp:72-79); the bit kinds reserve one symbol's bits
size_t group_in(const pcx_repack *h)
{
    const unsigned w = h->mod;
    switch (h->kind) {
    case PCX_REPACK_BITS_TO_SYMBOLS: return w;
    case PCX_REPACK_SYMBOLS_TO_BITS: return 1;
    case PCX_REPACK_BYTES_TO_SYMBOLS: return w == 3 || w == 5 || w == 7 ? w : w == 6 ? 3 : 1;
    }
    return w == 8 ? 1 : w == 4 ? 2 : w == 6 || w == 2 ? 4 : 8;
}
const char *kind_name(int kind)
{
    static const char *const names[] = {"bits to symbols", "symbols to bits", "bytes to symbols", "symbols to bytes"};
    return names[kind];
}
}  // namespace

int pcx_repack_create(int kind, pcx_repack **out)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(kind >= PCX_REPACK_BITS_TO_SYMBOLS && kind <= PCX_REPACK_SYMBOLS_TO_BYTES, "repack: unknown kind %d", kind);
    pcx_repack *h = new (std::nothrow) pcx_repack();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->kind = kind;
    h->mod = 1;
    h->msb = kind == PCX_REPACK_BITS_TO_SYMBOLS || kind == PCX_REPACK_SYMBOLS_TO_BITS;
    *out = h;
    return PCX_OK;
}
int pcx_repack_destroy(pcx_repack *h) { delete h; return PCX_OK; }

int pcx_repack_set_modulus(pcx_repack *h, unsigned mod)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(mod >= 1 && mod <= 8, "Modulus must be between 1 and 8 inclusive");
    h->mod = mod;
    return PCX_OK;
}
int pcx_repack_get_modulus(const pcx_repack *h, unsigned *mod)
{
    PCX_CHECK_ARG(h && mod, "null argument");
    *mod = h->mod;
    return PCX_OK;
}
int pcx_repack_set_bit_order(pcx_repack *h, int msb)
{
    PCX_CHECK_ARG(h, "null handle");
    h->msb = msb != 0;
    return PCX_OK;
}
int pcx_repack_get_bit_order(const pcx_repack *h, int *msb)
{
    PCX_CHECK_ARG(h && msb, "null argument");
    *msb = h->msb ? 1 : 0;
    return PCX_OK;
}
int pcx_repack_get_group(const pcx_repack *h, size_t *in_elems, size_t *out_elems)
{
    PCX_CHECK_ARG(h && in_elems && out_elems, "null argument");
    *in_elems = group_in(h);
    *out_elems = repack_out_elems(h->kind, h->mod, *in_elems);
    return PCX_OK;
}
int pcx_repack_get_geometry(const pcx_repack *h, size_t *tile, size_t *slice)
{
    PCX_CHECK_ARG(h && tile && slice, "null argument");
    *tile = repack_tile(h->kind, h->mod);
    *slice = repack_slice(h->kind, h->mod);
    return PCX_OK;
}

int pcx_repack_process_dev(pcx_repack *h, const void *in_dev, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(n % group_in(h) == 0, "%s: %zu elements are not a whole group of %zu", kind_name(h->kind), n, group_in(h));
    PCX_CHECK_ARG(in_dev && out_dev, "null buffer");
    PCX_CHECK_ARG(buffers_ok(in_dev, n, out_dev, repack_out_elems(h->kind, h->mod, n), false), "%s: out overlaps in", kind_name(h->kind));
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    const char *in = static_cast<const char *>(in_dev);
    char *out = static_cast<char *>(out_dev);
    const size_t slice = repack_slice(h->kind, h->mod);
    for (size_t off = 0; off < n; off += slice)
        PCX_TRY(launch_repack_slice(h->kind, h->mod, h->msb, in + off, out + repack_out_elems(h->kind, h->mod, off), std::min(slice, n - off), st));
    return PCX_OK;
}
int pcx_repack_process(pcx_repack *h, const void *in, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(n % group_in(h) == 0, "%s: %zu elements are not a whole group of %zu", kind_name(h->kind), n, group_in(h));
    PCX_CHECK_ARG(in && out, "null buffer");
    const size_t m = repack_out_elems(h->kind, h->mod, n);
    PCX_CHECK_ARG(buffers_ok(in, n, out, m, false), "%s: out overlaps in", kind_name(h->kind));
    DeviceScope dev_scope(h->cx.device);
    return host_call(h, in, n, out, m, [&](const void *din, void *dout, hipStream_t st) { return pcx_repack_process_dev(h, din, dout, n, st); });
}
