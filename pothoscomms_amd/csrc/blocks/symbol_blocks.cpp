// symbol_blocks.cpp -- the seventh module of this port: the four blocks of the reference's digital/ directory that join the bit side
// of a modem chain to its sample side, libpcx_symbol_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a
// PothosComms build this source joins the DigitalBlocks module.
//
//   /comms/symbol_mapper, /blocks/symbol_mapper                   digital/SymbolMapper.cpp:47-128
//   /comms/symbol_slicer, /blocks/symbol_slicer                   digital/SymbolSlicer.cpp:42-133
//   /comms/differential_encoder, /blocks/differential_encoder     digital/DifferentialEncoder.cpp:22-82
//   /comms/differential_decoder, /blocks/differential_decoder     digital/DifferentialDecoder.cpp:22-84
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;

namespace {

using namespace pcxblk;     // check, OnDevice, kDomain, parseElemType, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_symbols_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

// one map value into the stream type's scalar: floats by conversion, integers toward zero within the type's range (NaN -> 0).  A
// double holds integers exactly up to 2^53: an int64 map beyond that goes through pcx_mapper_set_map / pcx_slicer_set_map.
template <typename T>
void putScalar(unsigned char *dst, double v)
{
    T t;
    if (std::is_floating_point<T>::value) t = (T)v;
    else if (std::isnan(v)) t = 0;
    else if (v <= (double)std::numeric_limits<T>::min()) t = std::numeric_limits<T>::min();
    else if (v >= (double)std::numeric_limits<T>::max()) t = std::numeric_limits<T>::max();
    else t = (T)v;
    std::memcpy(dst, &t, sizeof(T));
}
template <typename T>
double getScalar(const unsigned char *src)
{
    T t;
    std::memcpy(&t, src, sizeof(T));
    return (double)t;
}
size_t scalarBytes(int scalar) { return scalar == PCX_F64 || scalar == PCX_I64 ? 8 : scalar == PCX_F32 || scalar == PCX_I32 ? 4 : scalar == PCX_I16 ? 2 : 1; }
void putScalar(int scalar, unsigned char *dst, double v)
{
    switch (scalar) {
    case PCX_F64: putScalar<double>(dst, v); break;
    case PCX_F32: putScalar<float>(dst, v); break;
    case PCX_I64: putScalar<int64_t>(dst, v); break;
    case PCX_I32: putScalar<int32_t>(dst, v); break;
    case PCX_I16: putScalar<int16_t>(dst, v); break;
    default: putScalar<int8_t>(dst, v);
    }
}
double getScalar(int scalar, const unsigned char *src)
{
    switch (scalar) {
    case PCX_F64: return getScalar<double>(src);
    case PCX_F32: return getScalar<float>(src);
    case PCX_I64: return getScalar<int64_t>(src);
    case PCX_I32: return getScalar<int32_t>(src);
    case PCX_I16: return getScalar<int16_t>(src);
    }
    return getScalar<int8_t>(src);
}

/***********************************************************************
 * |PothosDoc Symbol Mapper
 *
 * Turns every input byte into one constellation point on the GPU.  The low bits of the byte select an entry of the map and that
 * entry is written to the output stream unchanged.  How many bits count follows from the map: a map of four entries reads two.
 *
 * |category /Digital
 * |category /Symbol
 * |keywords map symbol mapper
 * |alias /blocks/symbol_mapper
 *
 * |param dtype[Data Type] Element type of the points the block writes.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param map[Symbol Map] One output value per symbol, in symbol order, each representable in the chosen element type.
 * The list needs 1, 2, 4, 8 ... entries; of a list longer than 256 only the first 256 can ever be selected.
 * |default [-1, 1]
 * |option [BPSK] \[-1, 1\]
 * |option [QPSK] \[-1.0-1.0*j, -1.0+1.0*j, 1.0+1.0*j, 1.0-1.0*j\]
 * |option [2-bit Gray Code] \[0, 1, 3, 2\]
 * |option [3-bit Gray Code] \[0, 1, 3, 2, 6, 7, 5, 4\]
 * |option [4-bit Gray Code] \[0, 1, 3, 2, 6, 7, 5, 4, 12, 13, 15, 14, 10, 11, 9, 8\]
 * |widget ComboBox(editable=true)
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more symbols per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/symbol_mapper(dtype)
 * |setter setMap(map)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
/***********************************************************************
 * |PothosDoc Symbol Slicer
 *
 * Decides on the GPU which constellation point every input sample lies closest to and writes that point's position in the
 * map as one byte.  Among equally close points the earliest in the map wins.  A sample whose distance to every point is
 * not a number, or infinite, is given symbol 0.
 *
 * |category /Digital
 * |category /Symbol
 * |keywords symbol slicer
 * |alias /blocks/symbol_slicer
 *
 * |param dtype[Data Type] Element type of the samples the block reads.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param map[Symbol Map] The decision points in symbol order, each representable in the chosen element type.
 * Any length but zero is accepted; positions beyond 255 are reported modulo 256.
 * |default [-1, 1]
 * |option [BPSK] \[-1, 1\]
 * |option [QPSK] \[-1.0-1.0*j, -1.0+1.0*j, 1.0+1.0*j, 1.0-1.0*j\]
 * |widget ComboBox(editable=true)
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more samples per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/symbol_slicer(dtype)
 * |setter setMap(map)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// one class for both: the mapper writes the stream type, the slicer reads it; maps cross as complex doubles and are narrowed here
class MapBlock : public PortBlock {
public:
    MapBlock(const DType &dtype, int scalar, bool cplx, bool slicer)
        : PortBlock(slicer ? "SymbolSlicer" : "SymbolMapper", kPortSlabBytes), _slicer(slicer), _scalar(scalar), _cplx(cplx), _m(nullptr), _s(nullptr)
    {
        create(_m, _s, _who + "Factory(" + dtype.toString() + ")");        // the map is {1}: SymbolMapper.cpp:58, SymbolSlicer.cpp:64
        Block::setupInput(0, slicer ? dtype : DType(typeid(unsigned char)), kDomain);
        Block::setupOutput(0, slicer ? DType(typeid(unsigned char)) : dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(MapBlock, getMap));
        this->registerCall(this, PCX_FCN_TUPLE(MapBlock, setMap));
        this->registerCall(this, PCX_FCN_TUPLE(MapBlock, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(MapBlock, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(MapBlock, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(MapBlock, getPortSlabBytes));
    }
    ~MapBlock() { destroy(_m, _s); }

    std::vector<std::complex<double>> getMap() const
    {
        size_t n = 0;
        check(_slicer ? pcx_slicer_get_map(_s, nullptr, 0, &n) : pcx_mapper_get_map(_m, nullptr, 0, &n), _who + "::getMap()");
        const size_t sb = scalarBytes(_scalar), es = sb * (_cplx ? 2 : 1);
        std::vector<unsigned char> raw(n * es);
        check(_slicer ? pcx_slicer_get_map(_s, raw.data(), n, &n) : pcx_mapper_get_map(_m, raw.data(), n, &n), _who + "::getMap()");
        std::vector<std::complex<double>> map(n);
        for (size_t i = 0; i < n; i++)
            map[i] = std::complex<double>(getScalar(_scalar, raw.data() + i * es), _cplx ? getScalar(_scalar, raw.data() + i * es + sb) : 0.0);
        return map;
    }
    // setMap (SymbolMapper.cpp:66-77, SymbolSlicer.cpp:72-76): the handle refuses an empty map, the mapper's one whose length is not a
    // power of two as well
    void setMap(const std::vector<std::complex<double>> &map)
    {
        const std::vector<unsigned char> raw = narrowed(map);
        setRaw(_m, _s, raw, map.size(), _who + "::setMap()");
    }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with the map
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "MapBlock::setDevice()");
        const std::vector<std::complex<double>> map = getMap();
        pcx_mapper *m = nullptr;
        pcx_slicer *s = nullptr;
        create(m, s, _who + "::setDevice()");
        try {
            setRaw(m, s, narrowed(map), map.size(), _who + "::setDevice()");
        } catch (...) {
            destroy(m, s);
            throw;
        }
        destroy(_m, _s);
        _m = m;
        _s = s;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (SymbolMapper.cpp:79-95, SymbolSlicer.cpp:78-101): min(in, out) elements, consumed and produced
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t n = std::min(inPort->elements(), outPort->elements());
        if (n == 0) return;
        const void *in = inPort->buffer().template as<const void *>();
        void *out = outPort->buffer().template as<void *>();
        check(_slicer ? pcx_slicer_process(_s, in, out, n) : pcx_mapper_process(_m, in, out, n), _who + "::work()");
        inPort->consume(n);
        outPort->produce(n);
    }

private:
    void create(pcx_mapper *&m, pcx_slicer *&s, const std::string &where) const
    {
        check(_slicer ? pcx_slicer_create(_scalar, _cplx ? 1 : 0, &s) : pcx_mapper_create(_scalar, _cplx ? 1 : 0, &m), where);
    }
    void destroy(pcx_mapper *m, pcx_slicer *s) const
    {
        if (m) pcx_mapper_destroy(m);
        if (s) pcx_slicer_destroy(s);
    }
    void setRaw(pcx_mapper *m, pcx_slicer *s, const std::vector<unsigned char> &raw, size_t n, const std::string &where) const
    {
        check(_slicer ? pcx_slicer_set_map(s, raw.data(), n) : pcx_mapper_set_map(m, raw.data(), n), where);
    }
    std::vector<unsigned char> narrowed(const std::vector<std::complex<double>> &map) const
    {
        const size_t sb = scalarBytes(_scalar), es = sb * (_cplx ? 2 : 1);
        std::vector<unsigned char> raw(map.size() * es + 1);       // (+1: a pointer to hand over for an empty map)
        for (size_t i = 0; i < map.size(); i++) {
            putScalar(_scalar, raw.data() + i * es, map[i].real());
            if (_cplx) putScalar(_scalar, raw.data() + i * es + sb, map[i].imag());
        }
        return raw;
    }
    const bool _slicer;
    const int _scalar;
    const bool _cplx;
    pcx_mapper *_m;
    pcx_slicer *_s;
};

/***********************************************************************
 * |PothosDoc Differential Encoder
 *
 * Sends the running sum of the input symbols, taken modulo the symbol count, on the GPU.  A receiver then needs only the
 * change from one symbol to the next, so a constant phase ambiguity of the channel drops out.  The last symbol sent is
 * remembered from one buffer to the next.
 *
 * |category /Digital
 * |alias /blocks/differential_encoder
 *
 * |param symbols How many distinct symbol values the stream uses, one symbol per byte.
 * |default 2
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more symbols per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/differential_encoder()
 * |setter setSymbols(symbols)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
/***********************************************************************
 * |PothosDoc Differential Decoder
 *
 * Undoes the Differential Encoder block on the GPU: every output is the difference between a received symbol and the one
 * before it, taken modulo the symbol count.  The last symbol received is remembered from one buffer to the next.
 *
 * |category /Digital
 * |alias /blocks/differential_decoder
 *
 * |param symbols How many distinct symbol values the stream uses, one symbol per byte.
 * |default 2
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more symbols per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/differential_decoder()
 * |setter setSymbols(symbols)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// one class for both: the handle knows which recurrence it runs
class DiffBlock : public PortBlock {
public:
    explicit DiffBlock(bool decode)
        : PortBlock(decode ? "DifferentialDecoder" : "DifferentialEncoder", kPortSlabBytes), _decode(decode), _symbols(2), _h(nullptr)
    {
        check(pcx_diffcode_create(decode ? 1 : 0, &_h), _who + "()");      // symbols 2, the carried byte 0: :30 of either file
        Block::setupInput(0, DType(typeid(unsigned char)), kDomain);
        Block::setupOutput(0, DType(typeid(unsigned char)), kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(DiffBlock, setSymbols));
        this->registerCall(this, PCX_FCN_TUPLE(DiffBlock, getSymbols));
        this->registerCall(this, PCX_FCN_TUPLE(DiffBlock, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(DiffBlock, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(DiffBlock, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(DiffBlock, getPortSlabBytes));
    }
    ~DiffBlock() { pcx_diffcode_destroy(_h); }

    // setSymbols (:37-40): the size_t narrows to the block's uint32_t as it does there.  DEVIATION: a value that narrows to 0 (a
    // division by zero in the reference) is refused and the previous one kept.
    void setSymbols(const size_t symbols)
    {
        check(pcx_diffcode_set_symbols(_h, (uint32_t)symbols), _who + "::setSymbols()");
        _symbols = (uint32_t)symbols;
    }
    size_t getSymbols() const { return _symbols; }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with the symbol
    // count, and the carried byte starts over
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "DiffBlock::setDevice()");
        pcx_diffcode *fresh = nullptr;
        check(pcx_diffcode_create(_decode ? 1 : 0, &fresh), _who + "::setDevice()");
        const int rc = pcx_diffcode_set_symbols(fresh, _symbols);
        if (rc != PCX_OK) { pcx_diffcode_destroy(fresh); check(rc, _who + "::setDevice()"); }
        pcx_diffcode_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (:42-73): min(in, out) bytes, consumed and produced
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t n = std::min(inPort->elements(), outPort->elements());
        if (n == 0) return;
        check(pcx_diffcode_process(_h, inPort->buffer().template as<const void *>(), outPort->buffer().template as<void *>(), n), _who + "::work()");
        inPort->consume(n);
        outPort->produce(n);
    }

private:
    const bool _decode;
    uint32_t _symbols;
    pcx_diffcode *_h;
};

// SymbolMapperFactory, SymbolSlicerFactory: the six element types of the reference, real and complex, scalar streams only
Block *SymbolMapperFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) return new MapBlock(dtype, scalar, cplx, false);
    throw InvalidArgumentException("SymbolMapperFactory(" + dtype.toString() + ")", "unsupported type");
}
Block *SymbolSlicerFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) return new MapBlock(dtype, scalar, cplx, true);
    throw InvalidArgumentException("SymbolSlicerFactory(" + dtype.toString() + ")", "unsupported type");
}
Block *DifferentialEncoderFactory() { return new DiffBlock(false); }
Block *DifferentialDecoderFactory() { return new DiffBlock(true); }
pcxfw::BlockRegistry registerSymbolMapper("/comms/symbol_mapper", &SymbolMapperFactory);
pcxfw::BlockRegistry registerSymbolMapperOldPath("/blocks/symbol_mapper", &SymbolMapperFactory);
pcxfw::BlockRegistry registerSymbolSlicer("/comms/symbol_slicer", &SymbolSlicerFactory);
pcxfw::BlockRegistry registerSymbolSlicerOldPath("/blocks/symbol_slicer", &SymbolSlicerFactory);
pcxfw::BlockRegistry registerDifferentialEncoder("/comms/differential_encoder", &DifferentialEncoderFactory);
pcxfw::BlockRegistry registerDifferentialEncoderOldPath("/blocks/differential_encoder", &DifferentialEncoderFactory);
pcxfw::BlockRegistry registerDifferentialDecoder("/comms/differential_decoder", &DifferentialDecoderFactory);
pcxfw::BlockRegistry registerDifferentialDecoderOldPath("/blocks/differential_decoder", &DifferentialDecoderFactory);

}  // namespace
