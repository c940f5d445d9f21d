// digital_blocks.cpp -- the fifth module of this port: the two LFSR blocks of the reference's digital/ directory,
// libpcx_digital_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source joins the
// DigitalBlocks module.
//
//   /comms/scrambler, /blocks/scrambler         digital/Scrambler.cpp:36-187
//   /comms/descrambler, /blocks/descrambler     digital/Descrambler.cpp:36-187
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
using pcxfw::RangeException;

namespace {

using namespace pcxblk;     // check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_scrambler_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

/***********************************************************************
 * |PothosDoc Scrambler
 *
 * Whitens a stream of bits on the GPU with a Galois shift register.  Every stream element carries one bit in its lowest
 * position.  In additive mode the register free-runs and its feedback bit is XORed onto the data.  In multiplicative mode
 * the scrambled bit is also fed back into the register, so the sequence depends on the data itself.
 *
 * |category /Digital
 * |keywords scrambler
 * |alias /blocks/scrambler
 *
 * |param mode[Scrambler Mode] Whether the register free-runs or is driven by the scrambled bits.
 * |option [Additive] "additive"
 * |option [Multiplicative] "multiplicative"
 * |default "multiplicative"
 *
 * |param poly[Polynomial] Feedback polynomial of the register, one bit per power of x; 0x19 stands for x^4 + x^3 + 1.
 * |default 0x19
 *
 * |param seed[Seed] Value loaded into the register whenever the polynomial or the seed is set.
 * |default 0x1
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more bits per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/scrambler()
 * |setter setPoly(poly)
 * |setter setMode(mode)
 * |setter setSeed(seed)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
/***********************************************************************
 * |PothosDoc Descrambler
 *
 * Undoes the Scrambler block on the GPU: given the same mode, polynomial and seed it returns the bits that went in.  Every
 * stream element carries one bit in its lowest position.  In multiplicative mode the register is driven by the received
 * bits rather than by the recovered ones.
 *
 * |category /Digital
 * |keywords descrambler
 * |alias /blocks/descrambler
 *
 * |param mode[Descrambler Mode] Whether the register free-runs or is driven by the received bits.
 * |option [Additive] "additive"
 * |option [Multiplicative] "multiplicative"
 * |default "multiplicative"
 *
 * |param poly[Polynomial] Feedback polynomial of the register, one bit per power of x; 0x19 stands for x^4 + x^3 + 1.
 * |default 0x19
 *
 * |param seed[Seed] Value loaded into the register whenever the polynomial or the seed is set.
 * |default 0x1
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more bits per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/descrambler()
 * |setter setPoly(poly)
 * |setter setMode(mode)
 * |setter setSeed(seed)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// one class for both: they differ in what the multiplicative mode feeds back, which the handle knows
class LfsrBlock : public PortBlock {
public:
    explicit LfsrBlock(bool descramble)
        : PortBlock(descramble ? "Descrambler" : "Scrambler", kPortSlabBytes), _descramble(descramble), _poly(0x19), _seed(1),
          _mode("multiplicative"), _h(nullptr)
    {
        check(pcx_scrambler_create(descramble ? 1 : 0, &_h), _who + "()");      // multiplicative, seed 1, setPoly(0x19): Scrambler.cpp:58-61
        Block::setupInput(0, DType(typeid(unsigned char)), kDomain);
        Block::setupOutput(0, DType(typeid(unsigned char)), kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, setPoly));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, poly));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, setSeed));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, seed));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, setMode));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, mode));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, setSync));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, sync));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(LfsrBlock, getPortSlabBytes));
    }
    ~LfsrBlock() { pcx_scrambler_destroy(_h); }

    // setPoly, setSeed (Scrambler.cpp:64-79): each loads the register again from both values
    void setPoly(const int64_t &polynomial)
    {
        check(pcx_scrambler_set_poly(_h, polynomial), _who + "::setPoly()");
        _poly = polynomial;
    }
    int64_t poly() const { return _poly; }
    void setSeed(const int64_t &seed)
    {
        check(pcx_scrambler_set_seed(_h, seed), _who + "::setSeed()");
        _seed = seed;
    }
    int64_t seed() const { return _seed; }
    // setMode (Scrambler.cpp:86-91): the register is left alone
    void setMode(const std::string &mode)
    {
        check(pcx_scrambler_set_mode(_h, modeCode(mode)), _who + "::set_mode()");
        _mode = mode;
    }
    std::string mode() const { return _mode; }
    // setSync (Scrambler.cpp:99-117): validated and stored, unused by work() there and here
    void setSync(const std::string &sync_word)
    {
        _sync = sync_word;
        if (_sync.size() > 64) throw RangeException(_who + "::set_sync()", "sync word max len 64 bits");
        for (const char c : _sync)
            if (c != '0' && c != '1') throw RangeException(_who + "::set_sync()", "sync word must be 0s and 1s: " + _sync);
    }
    std::string sync() const { return _sync; }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with the
    // polynomial, seed and mode, and the register starts over
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "LfsrBlock::setDevice()");
        pcx_scrambler *fresh = nullptr;
        check(pcx_scrambler_create(_descramble ? 1 : 0, &fresh), _who + "::setDevice()");
        int rc = pcx_scrambler_set_mode(fresh, modeCode(_mode));
        if (rc == PCX_OK) rc = pcx_scrambler_set_seed(fresh, _seed);
        if (rc == PCX_OK) rc = pcx_scrambler_set_poly(fresh, _poly);
        if (rc != PCX_OK) { pcx_scrambler_destroy(fresh); check(rc, _who + "::setDevice()"); }
        pcx_scrambler_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (Scrambler.cpp:154-181): min(in, out) elements, consumed and produced
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t n = std::min(inPort->elements(), outPort->elements());
        if (n == 0) return;
        check(pcx_scrambler_process(_h, inPort->buffer().template as<const void *>(), outPort->buffer().template as<void *>(), n), _who + "::work()");
        inPort->consume(n);
        outPort->produce(n);
    }

private:
    // the names the reference accepts; anything else is handed on as a code the ABI refuses (InvalidArgumentException)
    int modeCode(const std::string &mode) const
    {
        if (mode == "additive") return PCX_SCR_ADDITIVE;
        if (mode == "multiplicative") return PCX_SCR_MULTIPLICATIVE;
        throw InvalidArgumentException(_who + "::set_mode()", "unknown mode: " + mode);
    }
    const bool _descramble;
    int64_t _poly, _seed;
    std::string _mode, _sync;
    pcx_scrambler *_h;
};

Block *ScramblerFactory() { return new LfsrBlock(false); }
Block *DescramblerFactory() { return new LfsrBlock(true); }
pcxfw::BlockRegistry registerScrambler("/comms/scrambler", &ScramblerFactory);
pcxfw::BlockRegistry registerScramblerOldPath("/blocks/scrambler", &ScramblerFactory);
pcxfw::BlockRegistry registerDescrambler("/comms/descrambler", &DescramblerFactory);
pcxfw::BlockRegistry registerDescramblerOldPath("/blocks/descrambler", &DescramblerFactory);

}  // namespace
