// iir_blocks.cpp -- the fourth module of this port: the IIR filter of the reference's filter/ directory, libpcx_iir_blocks.so (with
// the runner ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source joins the FilterBlocks module beside
// filter_blocks.cpp.
//
//   /comms/iir_filter, /blocks/iir_filter     filter/IIRFilter.cpp:11-121
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
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

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_iir_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

/***********************************************************************
 * |PothosDoc IIR Filter
 *
 * Runs a recursive (infinite impulse response) filter over a stream on the GPU.  Every output is a weighted sum of the
 * current and recent inputs, minus a weighted sum of recent outputs, computed in double precision and converted back to
 * the element type of the stream.  A complex stream is filtered as two independent real streams.
 *
 * |category /Filter
 * |keywords iir filter taps highpass lowpass recursive gpu hip
 * |alias /blocks/iir_filter
 *
 * |param dtype[Data Type] Element type of the input and output streams.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param taps Coefficients of the recursion, numerator then denominator.
 * Give the feedforward coefficients b[0..N] followed by the feedback coefficients a[0..N], so the list always has an even
 * length of at most 66 (order 32).  An IIR Designer can also send them at runtime through its taps signal.
 * <ul>
 * <li>The first half are the feedforward (numerator) coefficients.</li>
 * <li>The second half are the feedback (denominator) coefficients, led by a[0].</li>
 * </ul>
 * |default [0.0676, 0.135, 0.0676, 1, -1.142, 0.412]
 *
 * |param waitTaps[Wait Taps] Hold the stream back until taps have arrived through setTaps().
 * Choose this when a designer supplies the coefficients after the topology starts.
 * |default false
 * |preview valid
 * |option [Enabled] true
 * |option [Disabled] false
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
 * |factory /comms/iir_filter(dtype)
 * |setter setTaps(taps)
 * |setter setWaitTaps(waitTaps)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class IIRFilter : public PortBlock {
public:
    IIRFilter(const DType &dtype, int scalar, bool cplx)
        : PortBlock("IIRFilter", kPortSlabBytes), _scalar(scalar), _cplx(cplx), _waitTapsMode(false), _waitTapsArmed(false), _h(nullptr)
    {
        check(pcx_iir_create(scalar, cplx ? 1 : 0, &_h), "IIRFilterFactory(" + dtype.toString() + ")");
        _taps = {0.0676, 0.135, 0.0676, 1, -1.142, 0.412};       // the handle's own default (IIRFilter.cpp:57)
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, setTaps));
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, getTaps));
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, setWaitTaps));
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, getWaitTaps));
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(IIRFilter, getPortSlabBytes));
    }
    ~IIRFilter() { pcx_iir_destroy(_h); }

    // setTaps (IIRFilter.cpp:63-69): the history starts over and an armed waitTaps is released
    void setTaps(const std::vector<double> &taps)
    {
        if (taps.empty()) throw InvalidArgumentException("IIRFilter::setTaps()", "Order cannot 0");
        check(pcx_iir_set_taps(_h, taps.data(), taps.size()), "IIRFilter::setTaps()");
        _taps = taps;
        _waitTapsArmed = false;
    }
    std::vector<double> getTaps() const { return _taps; }
    void setWaitTaps(const bool waitTaps) { _waitTapsMode = waitTaps; }
    bool getWaitTaps() const { return _waitTapsMode; }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with the taps,
    // and the history starts over
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "IIRFilter::setDevice()");
        pcx_iir *fresh = nullptr;
        check(pcx_iir_create(_scalar, _cplx ? 1 : 0, &fresh), "IIRFilter::setDevice()");
        const int rc = pcx_iir_set_taps(fresh, _taps.data(), _taps.size());
        if (rc != PCX_OK) { pcx_iir_destroy(fresh); check(rc, "IIRFilter::setDevice()"); }
        pcx_iir_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // activate (IIRFilter.cpp:77-80): the history back to zero, waitTaps armed
    void activate()
    {
        check(pcx_iir_reset(_h), "IIRFilter::activate()");
        _waitTapsArmed = _waitTapsMode;
    }
    // work (IIRFilter.cpp:82-99): nothing while armed, else minElements in and out
    void work()
    {
        if (_waitTapsArmed) return;
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t N = this->workInfo().minElements;
        if (N == 0) return;
        check(pcx_iir_process(_h, inPort->buffer().template as<const void *>(), outPort->buffer().template as<void *>(), N),
              "IIRFilter::work()");
        inPort->consume(N);
        outPort->produce(N);
    }

private:
    const int _scalar;
    const bool _cplx;
    std::vector<double> _taps;
    bool _waitTapsMode, _waitTapsArmed;
    pcx_iir *_h;
};

// IIRFilterFactory: the six element types of the reference, real and complex, scalar streams only
Block *IIRFilterFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) return new IIRFilter(dtype, scalar, cplx);
    throw InvalidArgumentException("IIRFilterFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerIIRFilter("/comms/iir_filter", &IIRFilterFactory);
pcxfw::BlockRegistry registerIIRFilterOldPath("/blocks/iir_filter", &IIRFilterFactory);

}  // namespace
