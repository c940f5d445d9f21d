// repack_blocks.cpp -- the eighth module of this port: the four blocks of the reference's digital/ directory that convert between
// bits, symbols and payload bytes, libpcx_repack_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a
// PothosComms build this source joins the DigitalBlocks module.
//
//   /comms/bits_to_symbols, /blocks/bits_to_symbols       digital/BitsToSymbols.cpp:40-166
//   /comms/symbols_to_bits, /blocks/symbols_to_bits       digital/SymbolsToBits.cpp:37-163
//   /comms/bytes_to_symbols, /blocks/bytes_to_symbols     digital/BytesToSymbols.cpp:35-180
//   /comms/symbols_to_bytes, /blocks/symbols_to_bytes     digital/SymbolsToBytes.cpp:38-183
//
// DEVIATION: the packet path of the four blocks (msgWork and the hasMessage() branch of work(), e.g. BytesToSymbols.cpp:91-135) is
// left out, in the bundled runtime (which has no messages) and in a Pothos build alike: the reference rounds a packet up to whole
// groups and reads past the payload's end to do so, which is undefined.  A message that reaches the input port stays queued.
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <cstdint>
#include <string>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;

namespace {

using namespace pcxblk;     // check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_repack_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

const char *const kNames[4] = {"BitsToSymbols", "SymbolsToBits", "BytesToSymbols", "SymbolsToBytes"};

/***********************************************************************
 * |PothosDoc Bits To Symbols
 *
 * Collects N one-bit inputs into every output symbol on the GPU.  An input byte stands for a set bit whenever it is not zero,
 * whatever its value.  With N of 8 the block turns a stream of bits into the bytes they spell.
 *
 * |category /Digital
 * |category /Symbol
 * |alias /blocks/bits_to_symbols
 *
 * |param N[Modulus] How many input bits make up one output symbol.
 * |default 2
 * |widget SpinBox(minimum=1, maximum=8)
 *
 * |param bitOrder[Bit Order] Which end of the symbol the first bit of a run goes to.
 * MSBit puts the first input on the highest of the N bits, LSBit puts it on the lowest.
 * |option [MSBit] "MSBit"
 * |option [LSBit] "LSBit"
 * |default "MSBit"
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more elements per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/bits_to_symbols()
 * |setter setModulus(N)
 * |setter setBitOrder(bitOrder)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
/***********************************************************************
 * |PothosDoc Symbols To Bits
 *
 * Writes the N low bits of every input symbol as N separate outputs on the GPU, each of them 0 or 1.  Whatever a symbol
 * carries above its N bits is ignored.  With N of 8 the block spells every byte out as its eight bits.
 *
 * |category /Digital
 * |category /Symbol
 * |alias /blocks/symbols_to_bits
 *
 * |param N[Modulus] How many bits of one input symbol are written out.
 * |default 2
 * |widget SpinBox(minimum=1, maximum=8)
 *
 * |param bitOrder[Bit Order] Which end of the symbol is written first.
 * MSBit starts with the highest of the N bits, LSBit starts with the lowest.
 * |option [MSBit] "MSBit"
 * |option [LSBit] "LSBit"
 * |default "MSBit"
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more elements per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/symbols_to_bits()
 * |setter setModulus(N)
 * |setter setBitOrder(bitOrder)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
/***********************************************************************
 * |PothosDoc Bytes to Symbols
 *
 * Cuts a stream of payload bytes into symbols of N bits on the GPU, one symbol per output byte and every one below 2 to the N.
 * Symbols may straddle two input bytes, so the block works on the shortest run of bytes that holds a whole number of symbols.
 *
 * |category /Digital
 * |category /Symbol
 * |keywords pack bit byte symbol chunk
 * |alias /blocks/bytes_to_symbols
 *
 * |param N[Modulus] How many bits of the payload go into one output symbol.
 * |default 2
 * |widget SpinBox(minimum=1, maximum=8)
 *
 * |param bitOrder[Bit Order] From which end the payload bytes are used up.
 * MSBit takes the highest bits of a byte for the first symbol, LSBit takes the lowest.
 * |option [MSBit] "MSBit"
 * |option [LSBit] "LSBit"
 * |default "MSBit"
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more elements per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/bytes_to_symbols()
 * |setter setModulus(N)
 * |setter setBitOrder(bitOrder)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
/***********************************************************************
 * |PothosDoc Symbols to Bytes
 *
 * Joins symbols of N bits, one per input byte, into payload bytes on the GPU.  The block expects symbols below 2 to the N and
 * does not clear what lies above: stray high bits of a symbol show up in the neighbouring symbols of the same output bytes.
 *
 * |category /Digital
 * |category /Symbol
 * |keywords pack bit byte symbol chunk
 * |alias /blocks/symbols_to_bytes
 *
 * |param N[Modulus] How many bits every input symbol contributes to the payload.
 * |default 2
 * |widget SpinBox(minimum=1, maximum=8)
 *
 * |param bitOrder[Bit Order] From which end the payload bytes are filled.
 * MSBit places the first symbol on the highest bits of a byte, LSBit places it on the lowest.
 * |option [MSBit] "MSBit"
 * |option [LSBit] "LSBit"
 * |default "MSBit"
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more elements per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/symbols_to_bytes()
 * |setter setModulus(N)
 * |setter setBitOrder(bitOrder)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// one class for the four: the handle knows which conversion it runs and which group the reference reserves for it
class RepackBlock : public PortBlock {
public:
    explicit RepackBlock(int kind) : PortBlock(kNames[kind], kPortSlabBytes), _kind(kind), _h(nullptr)
    {
        check(pcx_repack_create(kind, &_h), _who + "()");      // modulus 1; MSBit for the bit kinds, LSBit for the byte kinds
        Block::setupInput(0, DType(typeid(unsigned char)), kDomain);
        Block::setupOutput(0, DType(typeid(unsigned char)), kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, getModulus));
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, setModulus));
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, setBitOrder));
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, getBitOrder));
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(RepackBlock, getPortSlabBytes));
    }
    ~RepackBlock() { pcx_repack_destroy(_h); }


    // setModulus (:64-71 of BitsToSymbols.cpp, the same check in the other three): the handle refuses anything outside 1 ... 8 and
    // keeps the previous value.  The reference's parameter is an unsigned char; a size_t that would narrow into 1 ... 8 is refused here.
    void setModulus(const size_t mod)
    {
        check(pcx_repack_set_modulus(_h, mod > 255 ? 0u : (unsigned)mod), _who + "::setModulus()");
    }
    size_t getModulus() const
    {
        unsigned mod = 0;
        check(pcx_repack_get_modulus(_h, &mod), _who + "::getModulus()");
        return mod;
    }
    // setBitOrder (:78-83)
    void setBitOrder(const std::string &order)
    {
        if (order != "LSBit" && order != "MSBit") throw InvalidArgumentException(_who + "::setBitOrder()", "Order must be LSBit or MSBit");
        check(pcx_repack_set_bit_order(_h, order == "MSBit" ? 1 : 0), _who + "::setBitOrder()");
    }
    std::string getBitOrder() const
    {
        int msb = 0;
        check(pcx_repack_get_bit_order(_h, &msb), _who + "::getBitOrder()");
        return msb ? "MSBit" : "LSBit";
    }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with its settings
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "RepackBlock::setDevice()");
        unsigned mod = 1;
        int msb = 0;
        check(pcx_repack_get_modulus(_h, &mod), _who + "::setDevice()");
        check(pcx_repack_get_bit_order(_h, &msb), _who + "::setDevice()");
        pcx_repack *fresh = nullptr;
        check(pcx_repack_create(_kind, &fresh), _who + "::setDevice()");
        pcx_repack_set_modulus(fresh, mod);
        pcx_repack_set_bit_order(fresh, msb);
        pcx_repack_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (BitsToSymbols.cpp:114-146, SymbolsToBits.cpp:112-143, BytesToSymbols.cpp:121-156, SymbolsToBytes.cpp:124-159): the
    // reserve on every call (none for symbols -> bits), the input and the output space each rounded down to whole groups, the
    // smaller of the two converted
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        size_t gin = 1, gout = 1;
        check(pcx_repack_get_group(_h, &gin, &gout), _who + "::work()");
        if (_kind != PCX_REPACK_SYMBOLS_TO_BITS) inPort->setReserve(gin);
        const size_t groups = std::min(inPort->elements() / gin, outPort->elements() / gout);
        if (groups == 0) return;
        check(pcx_repack_process(_h, inPort->buffer().template as<const void *>(), outPort->buffer().template as<void *>(), groups * gin),
              _who + "::work()");
        inPort->consume(groups * gin);
        outPort->produce(groups * gout);
    }

    // propagateLabels (:148-155 of BitsToSymbols.cpp and its counterparts): index and width scaled by the kind's ratio
    void propagateLabels(const pcxfw::InputPort *port)
    {
        const size_t w = getModulus();
        const size_t mult = _kind == PCX_REPACK_BITS_TO_SYMBOLS ? 1 : _kind == PCX_REPACK_BYTES_TO_SYMBOLS ? 8 : w;
        const size_t div = _kind == PCX_REPACK_BITS_TO_SYMBOLS ? w : _kind == PCX_REPACK_BYTES_TO_SYMBOLS ? w : _kind == PCX_REPACK_SYMBOLS_TO_BITS ? 1 : 8;
        auto outPort = this->output(0);
        for (const auto &label : port->labels()) outPort->postLabel(label.toAdjusted(mult, div));
    }

private:
    const int _kind;
    pcx_repack *_h;
};

Block *BitsToSymbolsFactory() { return new RepackBlock(PCX_REPACK_BITS_TO_SYMBOLS); }
Block *SymbolsToBitsFactory() { return new RepackBlock(PCX_REPACK_SYMBOLS_TO_BITS); }
Block *BytesToSymbolsFactory() { return new RepackBlock(PCX_REPACK_BYTES_TO_SYMBOLS); }
Block *SymbolsToBytesFactory() { return new RepackBlock(PCX_REPACK_SYMBOLS_TO_BYTES); }
pcxfw::BlockRegistry registerBitsToSymbols("/comms/bits_to_symbols", &BitsToSymbolsFactory);
pcxfw::BlockRegistry registerBitsToSymbolsOldPath("/blocks/bits_to_symbols", &BitsToSymbolsFactory);
pcxfw::BlockRegistry registerSymbolsToBits("/comms/symbols_to_bits", &SymbolsToBitsFactory);
pcxfw::BlockRegistry registerSymbolsToBitsOldPath("/blocks/symbols_to_bits", &SymbolsToBitsFactory);
pcxfw::BlockRegistry registerBytesToSymbols("/comms/bytes_to_symbols", &BytesToSymbolsFactory);
pcxfw::BlockRegistry registerBytesToSymbolsOldPath("/blocks/bytes_to_symbols", &BytesToSymbolsFactory);
pcxfw::BlockRegistry registerSymbolsToBytes("/comms/symbols_to_bytes", &SymbolsToBytesFactory);
pcxfw::BlockRegistry registerSymbolsToBytesOldPath("/blocks/symbols_to_bytes", &SymbolsToBytesFactory);

}  // namespace
