// probe_blocks.cpp -- the fifteenth module of this port: libpcx_probe_blocks.so (with the runner ABI of include/pcx_blocks.h linked
// in).  In a PothosComms build this source joins the UtilityBlocks module.
//
//   /comms/signal_probe, /blocks/stream_probe     utility/SignalProbe.cpp:12-194
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <chrono>
#include <complex>
#include <cstdint>
#include <string>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;

namespace {

using namespace pcxblk;     // parseElemType, check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_probe_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

inline void toProbeType(const double (&v)[2], double &out) { out = v[0]; }
inline void toProbeType(const double (&v)[2], std::complex<double> &out) { out = std::complex<double>(v[0], v[1]); }

/***********************************************************************
 * |PothosDoc Signal Probe
 *
 * Ends a chain on the GPU with one number: of each window of the stream arriving on input 0 the block keeps either the final
 * element, the root of the mean squared magnitude, or the average, computed on the device in double precision over a fixed
 * summation tree, so that equal windows give equal bits.  The number is handed out three ways: the call "value" returns it,
 * the signal "valueChanged" carries it after every calculation, and the slot "probeValue" makes the signal "valueTriggered"
 * carry it on request.  The block has no output port.
 *
 * |category /Utility
 * |category /Event
 * |keywords rms average mean
 * |alias /blocks/stream_probe
 *
 * |param dtype[Data Type] Element type of the stream that input 0 takes.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param mode What a window is reduced to.
 * VALUE keeps the window's final element and suits a stream that changes slowly,
 * RMS gives the root of the mean squared magnitude, MEAN the average (per component on a complex stream).
 * |default "VALUE"
 * |option [Value] "VALUE"
 * |option [RMS] "RMS"
 * |option [Mean] "MEAN"
 *
 * |param rate Upper bound on calculations per second.
 * Windows that arrive sooner than the bound allows are consumed unseen.
 * With 0.0 every window that arrives is calculated.
 * |preview valid
 * |default 0.0
 *
 * |param window Length of a window in elements; at least 1.
 * |default 1024
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
 * |factory /comms/signal_probe(dtype)
 * |setter setMode(mode)
 * |setter setRate(rate)
 * |setter setWindow(window)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename ProbeType>
class SignalProbe : public PortBlock {
public:
    SignalProbe(const DType &dtype, int scalar, bool cplx)
        : PortBlock("SignalProbe", kPortSlabBytes), _scalar(scalar), _cplx(cplx), _value(0), _mode("VALUE"), _window(1024), _rate(0.0), _h(nullptr)
    {
        check(pcx_probe_create(&_h, scalar, cplx ? 1 : 0), "signalProbeFactory(" + dtype.toString() + ")");     // VALUE, 1024: SignalProbe.cpp:64-67
        Block::setupInput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, value));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, setMode));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, getMode));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, setWindow));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, getWindow));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, setRate));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, getRate));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(SignalProbe, getPortSlabBytes));
        this->registerProbe("value");
        this->registerSignal("valueChanged");
        this->input(0)->setReserve(1);
    }
    ~SignalProbe() { pcx_probe_destroy(_h); }

    ProbeType value() { return _value; }

    // any string is kept (SignalProbe.cpp:87-90); one that names no calculation leaves the value alone in work()
    void setMode(const std::string &mode)
    {
        const int code = modeCode(mode);
        if (code >= 0) check(pcx_probe_set_mode(_h, code), "SignalProbe::setMode()");
        _mode = mode;
    }
    std::string getMode() const { return _mode; }

    // DIFFERENCE: a window of 0 is refused; the reference accepts it and then reads x[N-1] with N = 0 (SignalProbe.cpp:141)
    void setWindow(const size_t window)
    {
        if (window == 0) throw InvalidArgumentException("SignalProbe::setWindow(0)", "the window cannot be 0");
        check(pcx_probe_set_window(_h, window), "SignalProbe::setWindow()");
        _window = window;
        this->input(0)->setReserve(window);
    }
    size_t getWindow() const { return _window; }

    void setRate(const double rate) { _rate = rate; }
    double getRate() const { return _rate; }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there and takes the
    // mode and the window along
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        OnDevice on(d, "SignalProbe::setDevice()");
        pcx_probe *fresh = nullptr;
        check(pcx_probe_create(&fresh, _scalar, _cplx ? 1 : 0), "SignalProbe::setDevice()");
        int rc = pcx_probe_set_window(fresh, _window);
        const int code = modeCode(_mode);
        if (rc == PCX_OK && code >= 0) rc = pcx_probe_set_mode(fresh, code);
        if (rc != PCX_OK) { pcx_probe_destroy(fresh); check(rc, "SignalProbe::setDevice()"); }
        pcx_probe_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    void activate() { _nextCalc = std::chrono::high_resolution_clock::now(); }     // SignalProbe.cpp:118-121

    // work (SignalProbe.cpp:123-163): N = min(window, elements) are consumed; unless the rate holds the call back, the window is
    // reduced on the device and the value signalled.  DIFFERENCE: a call without an element returns at once; the reference goes on
    // to read x[N-1] there.
    void work()
    {
        auto inPort = this->input(0);
        const size_t N = std::min(_window, inPort->elements());
        if (N == 0) return;
        const void *x = inPort->buffer().template as<const void *>();
        inPort->consume(N);

        const auto currentTime = std::chrono::high_resolution_clock::now();
        if (_rate != 0.0 && currentTime < _nextCalc) return;
        if (_rate != 0.0) {
            const auto tps = std::chrono::nanoseconds((long long)(1e9 / _rate));
            _nextCalc += std::chrono::duration_cast<std::chrono::high_resolution_clock::duration>(tps);
        }

        if (modeCode(_mode) >= 0) {
            double v[2] = {0.0, 0.0};
            size_t consumed = 0;
            check(pcx_probe_process(_h, x, N, v, &consumed), "SignalProbe::work()");
            toProbeType(v, _value);
        }
        this->emitSignal("valueChanged", _value);
    }

private:
    static int modeCode(const std::string &mode)
    {
        if (mode == "VALUE") return PCX_PROBE_VALUE;
        if (mode == "RMS") return PCX_PROBE_RMS;
        if (mode == "MEAN") return PCX_PROBE_MEAN;
        return -1;
    }

    const int _scalar;
    const bool _cplx;
    ProbeType _value;
    std::string _mode;
    size_t _window;
    double _rate;
    std::chrono::high_resolution_clock::time_point _nextCalc;
    pcx_probe *_h;
};

// signalProbeFactory (SignalProbe.cpp:176-188): the six signed and floating element types and their complex forms, scalar streams only
Block *signalProbeFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) {
        if (cplx) return new SignalProbe<std::complex<double>>(dtype, scalar, true);
        return new SignalProbe<double>(dtype, scalar, false);
    }
    throw InvalidArgumentException("signalProbeFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerSignalProbe("/comms/signal_probe", &signalProbeFactory);
pcxfw::BlockRegistry registerSignalProbeOldPath("/blocks/stream_probe", &signalProbeFactory);

}  // namespace
