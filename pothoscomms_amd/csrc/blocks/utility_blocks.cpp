// utility_blocks.cpp -- the tenth module of this port: the reference's utility/ directory, libpcx_utility_blocks.so (with the runner
// ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source joins the UtilityBlocks module.
//
//   /comms/threshold, /blocks/threshold     utility/Threshold.cpp:8-179
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

using namespace pcxblk;     // parseElemType, check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_threshold_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

/***********************************************************************
 * |PothosDoc Threshold
 *
 * Turns a level into events: the GPU compares every element of the stream arriving on input 0 with two levels and remembers
 * whether the signal is active.  An inactive signal becomes active at an element above the activation level, an active one
 * becomes inactive at an element below the deactivation level, and each such element receives a label.  The stream itself
 * leaves unchanged on output 0.  Behind an envelope detector this is a burst detector.
 *
 * |category /Utility
 * |keywords threshold activate level
 * |alias /blocks/threshold
 *
 * |param dtype[Data Type] Element type of the stream, the same on the input and on the output.
 * |widget DTypeChooser(float=1,int=1)
 * |default "float64"
 * |preview disable
 *
 * |param activationLevel[Activation Level] The level the input must exceed to activate.
 * |default 0.5
 *
 * |param deactivationLevel[Deactivation Level] The level the input must fall below to deactivate.
 * |default 0.5
 *
 * |param activationId[Activation ID] Name given to the label on the element that activates.
 * With an empty string no activation labels are produced.
 * |default ""
 * |widget StringEntry()
 * |preview valid
 *
 * |param deactivationId[Deactivation ID] Name given to the label on the element that deactivates.
 * With an empty string no deactivation labels are produced.
 * |default ""
 * |widget StringEntry()
 * |preview valid
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
 * |factory /comms/threshold(dtype)
 * |setter setActivationLevel(activationLevel)
 * |setter setDeactivationLevel(deactivationLevel)
 * |setter setActivationId(activationId)
 * |setter setDeactivationId(deactivationId)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename Type>
class Threshold : public PortBlock {
public:
    Threshold(const DType &dtype, int scalar)
        : PortBlock("Threshold", kPortSlabBytes), _scalar(scalar), _activationLevel(0), _deactivationLevel(0), _h(nullptr), _idx(4096)
    {
        check(pcx_threshold_create(&_h, scalar), "ThresholdFactory(" + dtype.toString() + ")");      // levels 0, inactive: Threshold.cpp:54-58
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, setActivationLevel));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, getActivationLevel));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, setDeactivationLevel));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, getDeactivationLevel));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, setActivationId));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, getActivationId));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, setDeactivationId));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, getDeactivationId));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(Threshold, getPortSlabBytes));
    }
    ~Threshold() { pcx_threshold_destroy(_h); }

    void setActivationLevel(const Type level)
    {
        check(pcx_threshold_set_levels(_h, &level, &_deactivationLevel), "Threshold::setActivationLevel()");
        _activationLevel = level;
    }
    Type getActivationLevel() const { return _activationLevel; }
    void setDeactivationLevel(const Type level)
    {
        check(pcx_threshold_set_levels(_h, &_activationLevel, &level), "Threshold::setDeactivationLevel()");
        _deactivationLevel = level;
    }
    Type getDeactivationLevel() const { return _deactivationLevel; }
    void setActivationId(const std::string &id) { _activationId = id; }
    std::string getActivationId() const { return _activationId; }
    void setDeactivationId(const std::string &id) { _deactivationId = id; }
    std::string getDeactivationId() const { return _deactivationId; }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there and takes the
    // levels and the state along
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        int state = 0;
        check(pcx_threshold_get_state(_h, &state), "Threshold::setDevice()");
        OnDevice on(d, "Threshold::setDevice()");
        pcx_threshold *fresh = nullptr;
        check(pcx_threshold_create(&fresh, _scalar), "Threshold::setDevice()");
        int rc = pcx_threshold_set_levels(fresh, &_activationLevel, &_deactivationLevel);
        if (rc == PCX_OK) rc = pcx_threshold_set_state(fresh, state);
        if (rc != PCX_OK) { pcx_threshold_destroy(fresh); check(rc, "Threshold::setDevice()"); }
        pcx_threshold_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // reset state before running (Threshold.cpp:111-115)
    void activate() { check(pcx_threshold_reset(_h), "Threshold::activate()"); }

    // work (Threshold.cpp:117-149).  The reference takes the input buffer and posts it on the output; here k = min(in, out)
    // elements are compared and copied into the output port's buffer by the same kernel.
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t k = std::min(inPort->elements(), outPort->elements());
        if (k == 0) return;
        const void *x = inPort->buffer().template as<const void *>();
        void *y = outPort->buffer().template as<void *>();
        size_t transitions = 0;
        int entry = 0;
        check(pcx_threshold_process(_h, x, k, y, _idx.data(), _idx.size(), &transitions, &entry), "Threshold::work()");
        if (transitions > _idx.size()) {
            // more transitions than the index buffer held.  The call has advanced the carried state: the buffer grows, the state
            // goes back to the one the call was entered in, and the call is made again
            _idx.resize(transitions);
            check(pcx_threshold_set_state(_h, entry), "Threshold::work()");
            check(pcx_threshold_process(_h, x, k, y, _idx.data(), _idx.size(), &transitions, &entry), "Threshold::work()");
        }
        // the two kinds alternate from the entry state on; a kind without an ID is skipped (Threshold.cpp:135, :141)
        for (size_t j = 0; j < transitions; j++) {
            const std::string &id = ((size_t)entry + j) % 2 == 0 ? _activationId : _deactivationId;
            if (!id.empty()) outPort->postLabel(pcxfw::Label(id, pcxfw::Object(), _idx[j], 1));
        }
        inPort->consume(k);
        outPort->produce(k);
    }

private:
    const int _scalar;
    Type _activationLevel, _deactivationLevel;
    std::string _activationId, _deactivationId;
    pcx_threshold *_h;
    std::vector<uint64_t> _idx;
};

// ThresholdFactory (Threshold.cpp:163-174): the six real element types, scalar streams only
Block *ThresholdFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && !cplx && dtype.dimension() == 1) {
        switch (scalar) {
        case PCX_F64: return new Threshold<double>(dtype, scalar);
        case PCX_F32: return new Threshold<float>(dtype, scalar);
        case PCX_I64: return new Threshold<int64_t>(dtype, scalar);
        case PCX_I32: return new Threshold<int32_t>(dtype, scalar);
        case PCX_I16: return new Threshold<int16_t>(dtype, scalar);
        case PCX_I8: return new Threshold<int8_t>(dtype, scalar);
        }
    }
    throw InvalidArgumentException("ThresholdFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerThreshold("/comms/threshold", &ThresholdFactory);
pcxfw::BlockRegistry registerThresholdOldPath("/blocks/threshold", &ThresholdFactory);

}  // namespace
