// pcx_src_api.hip -- the pcx_source handle (include/pcx.h) and the two host-only table builders of the waveform module.
//   pcx_source          the table as it was set and on the device, one period of the walk (seq, source.hip) and the carried index.  The
//                       index is host state: it advances when a call is made.  seq is written again only after a table, step or index
//                       was SET, by a kernel on the stream of the next generate call, so that call still allocates and awaits nothing.
//   pcx_waveform_table  updateTable() / setElem() of WaveformSource.cpp:178-259, in double and in the reference's order
//   pcx_noise           the std::mt19937 of NoiseSource.cpp and its distributions as :188-250 call them
#include <random>

#include "pcx_host.hpp"

using namespace pcx;

struct pcx_source {
    ExecCtx cx;
    int scalar = PCX_F32;
    bool cplx = false;
    size_t es = 4;                      // bytes of an element
    std::vector<unsigned char> table;   // as set
    size_t entries = 0;
    uint64_t step = 0, index = 0;
    size_t period = 0;                  // entries / gcd(step mod entries, entries)
    bool tab_ready = false;             // tab holds the table, seq is large enough
    bool seq_ready = false;             // seq holds the period that starts `since` elements behind the index
    uint64_t since = 0;
    DevBuf tab, seq;
    StageBuf wsOut;
};

namespace {

int source_prepare(pcx_source *h)
{
    if (h->tab_ready) return PCX_OK;
    PCX_TRY(ctx_quiesce(h->cx));        // an earlier call's kernels may still read the table and the period
    PCX_TRY(upload(h->tab, h->table));
    PCX_TRY(h->seq.ensure(source_seq_bytes(h->period, h->es)));
    h->tab_ready = true;
    h->seq_ready = false;
    return PCX_OK;
}
// elements of the period as seq holds it: written out to at least 16 bytes
size_t seq_elems(const pcx_source *h) { return std::max<size_t>(h->period, 16 / h->es); }

}  // namespace

int pcx_source_create(int scalar, int is_complex, pcx_source **out)
{
    PCX_CHECK_ARG(out, "null out");
    PCX_CHECK_ARG(valid_scalar(scalar), "source: unsupported type");
    pcx_source *h = new (std::nothrow) pcx_source();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    h->scalar = scalar;
    h->cplx = is_complex != 0;
    h->es = elem_bytes(scalar, h->cplx);
    if (device_reachable()) { DeviceScope bind(h->cx.device); }     // bound to the device current now
    *out = h;
    return PCX_OK;
}
int pcx_source_destroy(pcx_source *h) { delete h; return PCX_OK; }

int pcx_source_set_table(pcx_source *h, const void *table, size_t entries, uint64_t step)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(entries != 0 && (entries & (entries - 1)) == 0 && entries <= source_max_entries(),
                  "table size must be a power of two of at most %zu entries", source_max_entries());
    PCX_CHECK_ARG(table, "null table");
    const unsigned char *t = static_cast<const unsigned char *>(table);
    h->table.assign(t, t + entries * h->es);
    h->entries = entries;
    h->step = step;
    const uint64_t s = step & (entries - 1);
    h->period = s ? entries / (size_t)std::min<uint64_t>(s & (~s + 1), entries) : 1;     // the gcd with a power of two: the lowest set bit
    h->tab_ready = false;
    h->seq_ready = false;
    if (!device_reachable()) return PCX_OK;
    DeviceScope dev_scope(h->cx.device);
    return source_prepare(h);
}
int pcx_source_get_index(const pcx_source *h, uint64_t *index)
{
    PCX_CHECK_ARG(h && index, "null argument");
    *index = h->index;
    return PCX_OK;
}
int pcx_source_set_index(pcx_source *h, uint64_t index)
{
    PCX_CHECK_ARG(h, "null handle");
    // a walk of step 1 (the noise source, which moves its index in front of every call) reaches every index inside the period it has
    if (h->seq_ready && h->step == 1) h->since += index - h->index;
    else h->seq_ready = false;
    h->index = index;
    return PCX_OK;
}
int pcx_source_get_geometry(const pcx_source *h, size_t *tile, size_t *period, int *staged)
{
    PCX_CHECK_ARG(h && tile && period && staged, "null argument");
    *tile = source_tile_bytes() / h->es;
    *period = h->period;
    *staged = h->period && seq_elems(h) * h->es <= source_lds_bytes() ? 1 : 0;
    return PCX_OK;
}

int pcx_source_generate_dev(pcx_source *h, void *out_dev, size_t n, void *stream)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(out_dev, "null buffer");
    PCX_CHECK_ARG(n <= (~(size_t)0 >> 5), "source: %zu elements", n);
    if (!h->entries) { set_error("source: no table set"); return PCX_ERR_STATE; }
    DeviceScope dev_scope(h->cx.device);
    PCX_TRY(source_prepare(h));
    hipStream_t st = as_stream(stream);
    PCX_TRY(ctx_enter(h->cx, st));
    if (source_gather_selected()) {
        PCX_TRY(launch_source_gather(h->es, h->tab.p, out_dev, h->index, h->step, h->entries, n, st));
    } else {
        if (!h->seq_ready) {
            PCX_TRY(launch_source_permute(h->es, h->tab.p, h->seq.p, h->index, h->step, h->entries, h->period, st));
            h->seq_ready = true;
            h->since = 0;
        }
        const size_t q = seq_elems(h);
        PCX_TRY(launch_source_copy(h->seq.p, out_dev, n * h->es, (size_t)(h->since & (q - 1)) * h->es, q * h->es, st));
        h->since += n;
    }
    h->index += (uint64_t)n * h->step;
    return PCX_OK;
}
int pcx_source_generate(pcx_source *h, void *out, size_t n)
{
    PCX_TRACE();
    PCX_CHECK_ARG(h, "null handle");
    if (n == 0) return PCX_OK;
    PCX_CHECK_ARG(out, "null buffer");
    PCX_CHECK_ARG(n <= (~(size_t)0 >> 5), "source: %zu elements", n);
    if (!h->entries) { set_error("source: no table set"); return PCX_ERR_STATE; }
    DeviceScope dev_scope(h->cx.device);
    hipStream_t st;
    PCX_TRY(ctx_own_stream(h->cx, &st));
    const size_t bytes = n * h->es;
    void *dout;
    bool staged;
    PCX_TRY(stage_out_begin(out, bytes, h->wsOut, &dout, &staged));
    {
        LinkBound link(out, nullptr);
        PCX_TRY(pcx_source_generate_dev(h, dout, n, st));
    }
    return stage_out_end(out, bytes, h->wsOut, staged, st);
}

// ------------------------------------------------------------------------------------------------------------ waveform table
namespace {

// setElem (WaveformSource.cpp:249-259, NoiseSource.cpp:227-237): Type(...) of the complex value resp. of its real part
template <typename T>
void set_elem(T &out, const std::complex<double> &scalar, const std::complex<double> &val, const std::complex<double> &offset)
{
    out = T((scalar * val + offset).real());
}
template <typename T>
void set_elem(std::complex<T> &out, const std::complex<double> &scalar, const std::complex<double> &val, const std::complex<double> &offset)
{
    out = std::complex<T>(scalar * val + offset);
}

template <typename Type>
int wave_fill(int wave, std::complex<double> scalar, std::complex<double> offset, void *table, size_t size)
{
    Type *t = static_cast<Type *>(table);
    switch (wave) {
    case PCX_WAVE_CONST:
        for (size_t i = 0; i < size; i++) set_elem(t[i], scalar, 1.0, offset);
        return PCX_OK;
    case PCX_WAVE_SINE:
        // std::polar(1.0, theta) AS g++ COMPILES IT in the reference: cos and sin of one argument become one sincos call, and glibc's
        // sincos differs from its sin and cos in the last place for about one argument in a thousand (353 of the 262144 of a
        // 2^18-entry table).  Spelled out here, so that the table does not depend on which compiler builds this file.  sincos is a
        // GNU extension of <math.h>, not ISO C or C++: the table's bit-exactness rests on glibc, as the reference's own does.
        for (size_t i = 0; i < size; i++) {
            double s, c;
            ::sincos(2 * M_PI * i / size, &s, &c);
            set_elem(t[i], scalar, std::complex<double>(1.0 * c, 1.0 * s), offset);
        }
        return PCX_OK;
    case PCX_WAVE_RAMP:
        for (size_t i = 0; i < size; i++) {
            const size_t q = (i + (3 * size) / 4) % size;
            set_elem(t[i], scalar, std::complex<double>(2.0 * i / (size - 1) - 1.0, 2.0 * q / (size - 1) - 1.0), offset);
        }
        return PCX_OK;
    case PCX_WAVE_SQUARE:
        for (size_t i = 0; i < size; i++) {
            const size_t q = (i + (3 * size) / 4) % size;
            set_elem(t[i], scalar, std::complex<double>((i < size / 2) ? 0.0 : 1.0, (q < size / 2) ? 0.0 : 1.0), offset);
        }
        return PCX_OK;
    }
    return PCX_ERR_ARG;
}

// calls f.template operator()<Type>() for the element type of (scalar, cplx)
template <typename F>
int for_type(int scalar, bool cplx, F &&f)
{
    switch (scalar) {
    case PCX_F64: return cplx ? f(static_cast<std::complex<double> *>(nullptr)) : f(static_cast<double *>(nullptr));
    case PCX_F32: return cplx ? f(static_cast<std::complex<float> *>(nullptr)) : f(static_cast<float *>(nullptr));
    case PCX_I64: return cplx ? f(static_cast<std::complex<int64_t> *>(nullptr)) : f(static_cast<int64_t *>(nullptr));
    case PCX_I32: return cplx ? f(static_cast<std::complex<int32_t> *>(nullptr)) : f(static_cast<int32_t *>(nullptr));
    case PCX_I16: return cplx ? f(static_cast<std::complex<int16_t> *>(nullptr)) : f(static_cast<int16_t *>(nullptr));
    case PCX_I8: return cplx ? f(static_cast<std::complex<int8_t> *>(nullptr)) : f(static_cast<int8_t *>(nullptr));
    }
    return PCX_ERR_ARG;
}

}  // namespace

int pcx_waveform_table(int scalar, int is_complex, int wave, double rate, double freq, double res, double ampl_re, double ampl_im, double offset_re,
                       double offset_im, void *table, size_t cap, size_t *entries, uint64_t *step)
{
    PCX_CHECK_ARG(entries && step, "null argument");
    PCX_CHECK_ARG(valid_scalar(scalar), "waveformSourceFactory: unsupported type");
    // the size loop (:182-196); max_size() of the table's vector lies far above the 2^20 limit for every element type
    const double frac = ((res == 0.0) ? freq : res) / rate;
    size_t numEntries = 4096;
    while (true) {
        const long long delta = std::llround(frac * numEntries);
        if (frac == 0.0) break;
        if (size_t(std::llabs(delta)) >= 16) break;
        if (numEntries * 2 > source_max_entries()) break;
        numEntries *= 2;
    }
    const size_t st = size_t(std::llround((freq / rate) * numEntries));
    PCX_CHECK_ARG(!(st == 0 && freq != 0.0), "step size not achievable");
    PCX_CHECK_ARG(wave >= PCX_WAVE_CONST && wave <= PCX_WAVE_SQUARE, "unknown waveform setting");
    *entries = numEntries;
    *step = st;
    if (!table || !cap) return PCX_OK;
    PCX_CHECK_ARG(cap >= numEntries, "waveform table: room for %zu of %zu entries", cap, numEntries);
    const std::complex<double> ampl(ampl_re, ampl_im), offset(offset_re, offset_im);
    return for_type(scalar, is_complex != 0, [&](auto *tag) {
        return wave_fill<typename std::remove_pointer<decltype(tag)>::type>(wave, ampl, offset, table, numEntries);
    });
}

// ------------------------------------------------------------------------------------------------------------ noise generator
struct pcx_noise {
    std::mt19937 gen;
    std::uniform_int_distribution<size_t> waveIndex{0, PCX_NOISE_ENTRIES - 1};
};

namespace {

// one entry's two draws.  The reference writes std::complex<double>(d(gen), d(gen)) and leaves the order to its compiler; the compiled
// reference (g++, the oracle's flags) draws the IMAGINARY component first (tests/golden/make_source_golden.py records it as
// `noise_imag_first` of the fixture, tests/test_source_cpu.py holds this constant against it)
constexpr bool kImagFirst = true;
template <typename D>
std::complex<double> draw_pair(D &&d)
{
    const double first = d();
    const double second = d();
    return kImagFirst ? std::complex<double>(second, first) : std::complex<double>(first, second);
}

template <typename Type>
int noise_fill(pcx_noise *h, int wave, double mean, double b, std::complex<double> scalar, std::complex<double> offset, void *table)
{
    Type *t = static_cast<Type *>(table);
    std::mt19937 &gen = h->gen;
    switch (wave) {
    case PCX_NOISE_UNIFORM: {
        std::uniform_real_distribution<> uniform(mean - b, mean + b);
        for (size_t i = 0; i < PCX_NOISE_ENTRIES; i++) set_elem(t[i], scalar, draw_pair([&] { return uniform(gen); }), offset);
        return PCX_OK;
    }
    case PCX_NOISE_NORMAL: {
        std::normal_distribution<> normal(mean, b);
        for (size_t i = 0; i < PCX_NOISE_ENTRIES; i++) set_elem(t[i], scalar, draw_pair([&] { return normal(gen); }), offset);
        return PCX_OK;
    }
    case PCX_NOISE_LAPLACE: {
        // (:208-214, :244-250) the uniform distribution over (mean - b, mean + b), not over (-1/2, 1/2)
        std::uniform_real_distribution<> uniform(mean - b, mean + b);
        auto laplace = [&]() -> double {
            auto num = uniform(gen);
            if (num < 0) return mean + b * std::log(1 + num);
            else return mean - b * std::log(1 - num);
        };
        for (size_t i = 0; i < PCX_NOISE_ENTRIES; i++) set_elem(t[i], scalar, draw_pair(laplace), offset);
        return PCX_OK;
    }
    case PCX_NOISE_POISSON: {
        std::poisson_distribution<> poisson(mean);
        for (size_t i = 0; i < PCX_NOISE_ENTRIES; i++) set_elem(t[i], scalar, draw_pair([&] { return (double)poisson(gen); }), offset);
        return PCX_OK;
    }
    }
    return PCX_ERR_ARG;
}

}  // namespace

int pcx_noise_create(int use_seed, uint32_t seed, pcx_noise **out)
{
    PCX_CHECK_ARG(out, "null out");
    pcx_noise *h = new (std::nothrow) pcx_noise();
    if (!h) { set_error("out of memory"); return PCX_ERR_STATE; }
    if (use_seed) h->gen.seed(seed);
    else { std::random_device rd; h->gen.seed(rd()); }      // _gen(_rd()), NoiseSource.cpp:84
    *out = h;
    return PCX_OK;
}
int pcx_noise_destroy(pcx_noise *h) { delete h; return PCX_OK; }

int pcx_noise_table(pcx_noise *h, int scalar, int is_complex, int wave, double mean, double b, double ampl_re, double ampl_im, double offset_re,
                    double offset_im, void *table)
{
    PCX_CHECK_ARG(h, "null handle");
    PCX_CHECK_ARG(valid_scalar(scalar), "noiseSourceFactory: unsupported type");
    PCX_CHECK_ARG(wave >= PCX_NOISE_UNIFORM && wave <= PCX_NOISE_POISSON, "unknown waveform setting");
    PCX_CHECK_ARG(table, "null table");
    const std::complex<double> ampl(ampl_re, ampl_im), offset(offset_re, offset_im);
    return for_type(scalar, is_complex != 0, [&](auto *tag) {
        return noise_fill<typename std::remove_pointer<decltype(tag)>::type>(h, wave, mean, b, ampl, offset, table);
    });
}
int pcx_noise_next_offset(pcx_noise *h, size_t *draw)
{
    PCX_CHECK_ARG(h && draw, "null argument");
    *draw = h->waveIndex(h->gen);
    return PCX_OK;
}
