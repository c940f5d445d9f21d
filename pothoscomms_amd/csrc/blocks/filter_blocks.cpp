// filter_blocks.cpp -- the second module of this port: the MI355X-backed blocks of the reference's FilterBlocks module that are not
// in comms_blocks.cpp.  Pothos builds one module library per source directory of the reference; this one is
// libpcx_filter_blocks.so (with the runner ABI of include/pcx_blocks.h linked in, so that hosts without PothosCore drive it the
// same way as libpcx_blocks.so).
//
//   /comms/dc_removal                          filter/DCRemoval.cpp:39-136
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <string>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;

namespace {

using namespace pcxblk;     // parseElemType, check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_dcremoval_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

/***********************************************************************
 * |PothosDoc DC Removal
 *
 * Subtracts the running DC level from a stream on the GPU.  The level is estimated by a chain of box-car averages,
 * each over the same number of samples; the output is the input, delayed to the centre of the first average, minus
 * the estimate.  History and accumulators carry over from one buffer to the next and start from zero on activation.
 * Integer streams give the same bits as the CPU block of PothosComms, wrap-around included; floating-point streams
 * are computed without the rounding drift of a running floating-point sum.
 *
 * |category /Filter
 * |keywords filter dc blocker bias gpu hip
 *
 * |param dtype[Data Type] Element type of the input and of the output stream.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param averageSize[Average Size] How many samples each box-car average spans.
 * A longer average follows the level more slowly and narrows the notch around zero frequency.
 * |default 512
 * |units samples
 *
 * |param cascadeSize[Cascade Size] How many box-car averages are chained.
 * Each extra stage steepens the notch edges and adds one more average of delay.
 * |default 2
 * |units filters
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
 * |factory /comms/dc_removal(dtype)
 * |setter setAverageSize(averageSize)
 * |setter setCascadeSize(cascadeSize)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class DCRemoval : public PortBlock {
public:
    DCRemoval(const DType &dtype, int scalar, bool cplx)
        : PortBlock("DCRemoval", kPortSlabBytes), _scalar(scalar), _cplx(cplx), _averageSize(512), _cascadeSize(2), _h(nullptr)
    {
        check(pcx_dcremoval_create(scalar, cplx ? 1 : 0, &_h), "DCRemovalFactory(" + dtype.toString() + ")");
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, setAverageSize));
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, getAverageSize));
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, setCascadeSize));
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, getCascadeSize));
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(DCRemoval, getPortSlabBytes));
    }
    ~DCRemoval() { pcx_dcremoval_destroy(_h); }

    void setAverageSize(const size_t num)
    {
        if (num == 0) throw InvalidArgumentException("DCRemoval::setAverageSize()", "average size cannot be zero");
        resize(num, _cascadeSize, "DCRemoval::setAverageSize()");
    }
    size_t getAverageSize() const { return _averageSize; }
    void setCascadeSize(const size_t num)
    {
        if (num == 0) throw InvalidArgumentException("DCRemoval::setCascadeSize()", "cascade size cannot be zero");
        resize(_averageSize, num, "DCRemoval::setCascadeSize()");
    }
    size_t getCascadeSize() const { return _cascadeSize; }

    // EXTENSION (as every block of comms_blocks.cpp): the GPU that carries the block; the handle is created again there and the
    // carried state starts over, as after activate()
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "DCRemoval::setDevice()");
        pcx_dcremoval *fresh = nullptr;
        check(pcx_dcremoval_create(_scalar, _cplx ? 1 : 0, &fresh), "DCRemoval::setDevice()");
        const int rc = pcx_dcremoval_set_sizes(fresh, _averageSize, _cascadeSize);
        if (rc != PCX_OK) { pcx_dcremoval_destroy(fresh); check(rc, "DCRemoval::setDevice()"); }
        pcx_dcremoval_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    void activate() { check(pcx_dcremoval_reset(_h), "DCRemoval::activate()"); }
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t N = this->workInfo().minElements;
        if (N == 0) return;
        check(pcx_dcremoval_process(_h, inPort->buffer().template as<const void *>(), outPort->buffer().template as<void *>(), N),
              "DCRemoval::work()");
        inPort->consume(N);
        outPort->produce(N);
    }

private:
    // new sizes, or (when the handle cannot allocate for them) the previous ones again, so that the block stays usable
    void resize(size_t average, size_t cascade, const char *where)
    {
        const int rc = pcx_dcremoval_set_sizes(_h, average, cascade);
        if (rc == PCX_OK) {
            _averageSize = average;
            _cascadeSize = cascade;
            return;
        }
        const std::string msg = pcx_last_error();
        (void)pcx_dcremoval_set_sizes(_h, _averageSize, _cascadeSize);
        if (rc == PCX_ERR_ARG) throw InvalidArgumentException(where, msg);
        throw pcxfw::Exception(where, msg);
    }
    const int _scalar;
    const bool _cplx;
    size_t _averageSize, _cascadeSize;
    pcx_dcremoval *_h;
};

// DCRemovalFactory: the six element types of the reference, real and complex, scalar streams only
Block *DCRemovalFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) return new DCRemoval(dtype, scalar, cplx);
    throw InvalidArgumentException("DCRemovalFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerDCRemoval("/comms/dc_removal", &DCRemovalFactory);

}  // namespace
