// correlator_blocks.cpp -- the sixth module of this port: the frame-start search of the reference's digital/ directory,
// libpcx_correlator_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source joins the
// DigitalBlocks module.
//
//   /comms/preamble_correlator, /blocks/preamble_correlator     digital/PreambleCorrelator.cpp:52-169
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;

namespace {

using namespace pcxblk;     // check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_preamble_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

/***********************************************************************
 * |PothosDoc Preamble Correlator
 *
 * Finds where frames start: the GPU slides a known symbol pattern along the stream arriving on input 0 and counts, at every
 * offset, how many bits of the stream differ from the pattern.  Wherever that count stays within the threshold, a label is
 * attached to the symbol that follows the pattern.  The stream itself leaves unchanged on output 0.
 *
 * Symbols are compared as whole bytes, so any symbol width up to eight bits works.  A stream of single bits is the special
 * case of one-bit symbols; its upper seven bits have to be zero to match a pattern of zeros and ones.
 *
 * http://en.wikipedia.org/wiki/Hamming_distance
 *
 * |category /Digital
 * |keywords bit symbol preamble correlate
 * |alias /blocks/preamble_correlator
 *
 * |param preamble The symbol pattern to look for, one entry per symbol, each as wide as the symbols of the stream.
 * |default [1]
 *
 * |param thresh[Threshold] Largest number of differing bits that still counts as a match.
 * A block whose threshold was never set runs with 1.
 * |default 0
 *
 * |param frameStartId[Frame Start ID] Name given to the label on the first symbol behind a matched pattern.
 * |default "frameStart"
 * |widget StringEntry()
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
 * |factory /comms/preamble_correlator()
 * |setter setPreamble(preamble)
 * |setter setThreshold(thresh)
 * |setter setFrameStartId(frameStartId)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class PreambleCorrelator : public PortBlock {
public:
    PreambleCorrelator()
        : PortBlock("PreambleCorrelator", kPortSlabBytes), _preamble(1, 1), _threshold(1), _frameStartId("frameStart"), _h(nullptr), _idx(4096)
    {
        check(pcx_preamble_create(&_h), "PreambleCorrelator()");      // preamble {1}, threshold 1: PreambleCorrelator.cpp:72-73
        Block::setupInput(0, DType(typeid(unsigned char)), kDomain);
        Block::setupOutput(0, DType(typeid(unsigned char)), kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, setPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, getPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, setThreshold));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, getThreshold));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, setFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, getFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleCorrelator, getPortSlabBytes));
    }
    ~PreambleCorrelator() { pcx_preamble_destroy(_h); }

    // setPreamble (PreambleCorrelator.cpp:77-81)
    void setPreamble(const std::vector<unsigned char> preamble)
    {
        check(pcx_preamble_set_preamble(_h, preamble.data(), preamble.size()), "PreambleCorrelator::setPreamble()");
        _preamble = preamble;
    }
    std::vector<unsigned char> getPreamble() const { return _preamble; }
    void setThreshold(const unsigned threshold)
    {
        check(pcx_preamble_set_threshold(_h, threshold), "PreambleCorrelator::setThreshold()");
        _threshold = threshold;
    }
    unsigned getThreshold() const { return _threshold; }
    void setFrameStartId(std::string id) { _frameStartId = id; }
    std::string getFrameStartId() const { return _frameStartId; }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "PreambleCorrelator::setDevice()");
        pcx_preamble *fresh = nullptr;
        check(pcx_preamble_create(&fresh), "PreambleCorrelator::setDevice()");
        int rc = pcx_preamble_set_preamble(fresh, _preamble.data(), _preamble.size());
        if (rc == PCX_OK) rc = pcx_preamble_set_threshold(fresh, _threshold);
        if (rc != PCX_OK) { pcx_preamble_destroy(fresh); check(rc, "PreambleCorrelator::setDevice()"); }
        pcx_preamble_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (PreambleCorrelator.cpp:114-154).  The reference takes the input buffer and posts it on the output; here k = min(in - P,
    // out) symbols are searched and copied into the output port's buffer by the same kernel.  A label index is
    // relative to the symbols this call produces and may lie up to P - 1 behind them, as in the reference.
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t P = _preamble.size();
        inPort->setReserve(P + 1);
        const size_t in = inPort->elements();
        if (in <= P) return;
        const size_t k = std::min(in - P, outPort->elements());
        if (k == 0) return;
        const void *x = inPort->buffer().template as<const void *>();
        void *y = outPort->buffer().template as<void *>();
        size_t positions = 0, matches = 0;
        check(pcx_preamble_process(_h, x, k + P, y, _idx.data(), _idx.size(), &positions, &matches), "PreambleCorrelator::work()");
        if (matches > _idx.size()) {          // more matches than the index buffer held: it grows and the call is made again
            _idx.resize(matches);
            check(pcx_preamble_process(_h, x, k + P, y, _idx.data(), _idx.size(), &positions, &matches), "PreambleCorrelator::work()");
        }
        for (size_t i = 0; i < matches; i++) outPort->postLabel(pcxfw::Label(_frameStartId, pcxfw::Object(), _idx[i], 1));
        inPort->consume(positions);
        outPort->produce(positions);
    }

private:
    std::vector<unsigned char> _preamble;
    unsigned _threshold;
    std::string _frameStartId;
    pcx_preamble *_h;
    std::vector<uint64_t> _idx;
};

Block *PreambleCorrelatorFactory() { return new PreambleCorrelator(); }
pcxfw::BlockRegistry registerPreambleCorrelator("/comms/preamble_correlator", &PreambleCorrelatorFactory);
pcxfw::BlockRegistry registerPreambleCorrelatorOldPath("/blocks/preamble_correlator", &PreambleCorrelatorFactory);

}  // namespace
