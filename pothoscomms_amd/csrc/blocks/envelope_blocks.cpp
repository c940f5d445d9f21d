// envelope_blocks.cpp -- the third module of this port: the envelope detector of the reference's filter/ directory,
// libpcx_envelope_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source joins the
// FilterBlocks module beside filter_blocks.cpp.
//
//   /comms/envelope_detector, /blocks/envelope_detector     filter/EnvelopeDetector.cpp:12-180
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <string>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;

namespace {

using namespace pcxblk;     // parseElemType, check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_envelope_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

/***********************************************************************
 * |PothosDoc Envelope Detector
 *
 * Follows the amplitude of a stream on the GPU with a one-pole smoother that rises at one rate and falls at another.
 * Each sample's magnitude is compared with the running envelope: above it, the envelope moves towards it at the
 * attack rate, otherwise at the release rate.  Real and complex streams of integers or floats are accepted, and the
 * envelope always leaves as float32, with the same bits as the CPU block of PothosComms.
 *
 * |category /Filter
 * |keywords filter envelope attack decay sustain release lookahead gpu hip
 * |alias /blocks/envelope_detector
 *
 * |param dtype[Input Type] Element type of the input stream.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param attack Time constant of a rising envelope, in samples.
 * The attack gain is exp(-1/attack); larger values rise more slowly.
 * |default 10
 * |units samples
 *
 * |param release Time constant of a falling envelope, in samples.
 * The release gain is exp(-1/release); larger values fall more slowly.
 * |default 10
 * |units samples
 *
 * |param lookahead How many samples ahead of the output the magnitude is read.
 * Reading ahead offsets the delay the smoothing introduces, so that the envelope lines up with the events of the stream.
 * |default 10
 * |units samples
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
 * |factory /comms/envelope_detector(dtype)
 * |setter setAttack(attack)
 * |setter setRelease(release)
 * |setter setLookahead(lookahead)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class EnvelopeDetector : public PortBlock {
public:
    EnvelopeDetector(const DType &dtype, int scalar, bool cplx)
        : PortBlock("EnvelopeDetector", kPortSlabBytes), _scalar(scalar), _cplx(cplx), _attack(0), _release(0), _lookahead(0), _h(nullptr)
    {
        check(pcx_envelope_create(scalar, cplx ? 1 : 0, &_h), "EnvelopeDetectorFactory(" + dtype.toString() + ")");
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, DType("float32"), kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, setAttack));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, getAttack));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, setRelease));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, getRelease));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, setLookahead));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, getLookahead));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(EnvelopeDetector, getPortSlabBytes));
    }
    ~EnvelopeDetector() { pcx_envelope_destroy(_h); }

    void setAttack(const float attack)
    {
        check(pcx_envelope_set_attack(_h, attack), "EnvelopeDetector::setAttack()");
        _attack = attack;
        _attackSet = true;
    }
    float getAttack() const { return _attack; }
    void setRelease(const float release)
    {
        check(pcx_envelope_set_release(_h, release), "EnvelopeDetector::setRelease()");
        _release = release;
        _releaseSet = true;
    }
    float getRelease() const { return _release; }
    void setLookahead(const size_t lookahead)
    {
        check(pcx_envelope_set_lookahead(_h, lookahead), "EnvelopeDetector::setLookahead()");
        _lookahead = lookahead;
    }
    size_t getLookahead() const { return _lookahead; }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there, the gains and
    // the lookahead pushed again, and the envelope starts over from 0
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "EnvelopeDetector::setDevice()");
        pcx_envelope *fresh = nullptr;
        check(pcx_envelope_create(_scalar, _cplx ? 1 : 0, &fresh), "EnvelopeDetector::setDevice()");
        // a setter that was never called leaves its gains at 0, as the reference's constructor does
        int rc = PCX_OK;
        if (_attackSet) rc = pcx_envelope_set_attack(fresh, _attack);
        if (rc == PCX_OK && _releaseSet) rc = pcx_envelope_set_release(fresh, _release);
        if (rc == PCX_OK) rc = pcx_envelope_set_lookahead(fresh, _lookahead);
        if (rc != PCX_OK) { pcx_envelope_destroy(fresh); check(rc, "EnvelopeDetector::setDevice()"); }
        pcx_envelope_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // no activate(): the envelope survives deactivate / activate, as in the reference
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        // the lookahead window must be in the buffer ahead of the first output
        if (inPort->elements() <= _lookahead) {
            inPort->setReserve(_lookahead + 1);
            return;
        }
        const size_t N = std::min(inPort->elements() - _lookahead, outPort->elements());
        if (N == 0) return;
        check(pcx_envelope_process(_h, inPort->buffer().template as<const void *>(), outPort->buffer().template as<void *>(), N),
              "EnvelopeDetector::work()");
        inPort->consume(N);
        outPort->produce(N);
    }

    // the lookahead window stays contiguous in front of new samples: the framework's circular buffer (EnvelopeDetector.cpp:151-154)
    // -- in the bundled runtime page-locked towards host blocks and in device memory between two blocks of this port, as the FIR's
    pcxfw::BufferManager::Sptr getInputBufferManager(const std::string &, const std::string &domain)
    {
#ifndef PCX_WITH_POTHOS
        if (domain == kDomain) {
            OnDevice on(_device, "EnvelopeDetector::getInputBufferManager()");
            return manager(true, "circular");
        }
        return manager(false, "circular");
#else
        (void)domain;
        return Pothos::BufferManager::make("circular");
#endif
    }

private:
    const int _scalar;
    const bool _cplx;
    float _attack, _release;
    bool _attackSet = false, _releaseSet = false;
    size_t _lookahead;
    pcx_envelope *_h;
};

// EnvelopeDetectorFactory: the six element types of the reference, real and complex, scalar streams only
Block *EnvelopeDetectorFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) return new EnvelopeDetector(dtype, scalar, cplx);
    throw InvalidArgumentException("EnvelopeDetectorFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerEnvelopeDetector("/comms/envelope_detector", &EnvelopeDetectorFactory);
pcxfw::BlockRegistry registerEnvelopeDetectorOldPath("/blocks/envelope_detector", &EnvelopeDetectorFactory);

}  // namespace
