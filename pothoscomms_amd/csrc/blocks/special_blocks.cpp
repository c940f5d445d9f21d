// special_blocks.cpp -- the fourteenth module of this port, libpcx_special_blocks.so (with the runner ABI of include/pcx_blocks.h linked
// in): the special-function blocks that complete the reference's math/ directory.  In a PothosComms build they join the MathBlocks
// module.
//
//   /comms/gamma lngamma                  math/Gamma.cpp:59-157
//   /comms/erf erfc                       math/ErrorFunction.cpp:62-155
//   /comms/beta                           math/Beta.cpp:52-122
//   /comms/modf                           math/ModF.cpp:43-117
//
// float32 and float64, at any dimension: all four work() functions of the reference hand their loop elems times the dimension.
//
// The maps are stateless calls of include/pcx.h (csrc/specfn.hip): a block holds the element type, what it computes and the device it
// runs on.  Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
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

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_specfn_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

// what the six blocks share: the element type and the device / port-slab extension
class SpecialBlock : public PortBlock {
public:
    SpecialBlock(const std::string &who, int scalar) : PortBlock(who, kPortSlabBytes), _where(who + "::work()"), _scalar(scalar)
    {
        this->registerCall(this, PCX_FCN_TUPLE(SpecialBlock, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(SpecialBlock, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(SpecialBlock, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(SpecialBlock, getPortSlabBytes));
    }
    void setDevice(const size_t device) { _device = checkedDevice(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

protected:
    const std::string _where;
    const int _scalar;
};

// one input, one output, one function of pcx_spec_fn (Gamma.cpp:69-82, ErrorFunction.cpp:71-84)
class Unary : public SpecialBlock {
public:
    Unary(const std::string &who, const DType &dtype, int scalar, int fn) : SpecialBlock(who, scalar), _fn(fn)
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
    }
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t n = elems * inPort->dtype().dimension();
        OnDevice on(_device, _where.c_str());
        check(pcx_specfn(_scalar, _fn, inPort->buffer().template as<const void *>(), outPort->buffer().template as<void *>(), n), _where);
        inPort->consume(elems);
        outPort->produce(elems);
    }

private:
    const int _fn;
};

// two indexed inputs, one output (Beta.cpp:62-77): the shorter input decides
class Beta : public SpecialBlock {
public:
    Beta(const DType &dtype, int scalar) : SpecialBlock("Beta", scalar)
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupInput(1, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
    }
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto in0 = this->input(0);
        auto in1 = this->input(1);
        auto outPort = this->output(0);
        const size_t n = elems * in0->dtype().dimension();
        OnDevice on(_device, _where.c_str());
        check(pcx_beta(_scalar, in0->buffer().template as<const void *>(), in1->buffer().template as<const void *>(),
                       outPort->buffer().template as<void *>(), n),
              _where);
        in0->consume(elems);
        in1->consume(elems);
        outPort->produce(elems);
    }
};

// input 0, the named outputs "int" and "frac" (ModF.cpp:68-94)
class ModF : public SpecialBlock {
public:
    ModF(const DType &dtype, int scalar) : SpecialBlock("ModF", scalar)
    {
        Block::setupInput(0, dtype, kDomain);
        _intPort = Block::setupOutput("int", dtype, kDomain);
        _fracPort = Block::setupOutput("frac", dtype, kDomain);
    }
    void work()
    {
        const size_t elems = this->workInfo().minAllElements;
        if (elems == 0) return;
        auto inPort = this->input(0);
        const size_t n = elems * inPort->dtype().dimension();
        OnDevice on(_device, _where.c_str());
        check(pcx_modf(_scalar, inPort->buffer().template as<const void *>(), _intPort->buffer().template as<void *>(),
                       _fracPort->buffer().template as<void *>(), n),
              _where);
        inPort->consume(elems);
        _intPort->produce(elems);
        _fracPort->produce(elems);
    }

private:
    pcxfw::OutputPort *_intPort;
    pcxfw::OutputPort *_fracPort;
};

bool isFloat(const DType &dtype, int &scalar)
{
    bool cplx;
    return parseElemType(dtype, scalar, cplx) && !cplx && (scalar == PCX_F64 || scalar == PCX_F32);
}

/***********************************************************************
 * |PothosDoc Gamma
 *
 * Evaluates Euler's gamma function at every element of a stream on the GPU.  A float32 element is widened, taken through the
 * double-precision function and rounded once.  A zero gives the infinity of its sign, a negative integer gives a NaN.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output: float32 or float64.
 * |widget DTypeChooser(float=1)
 * |default "float64"
 * |preview disable
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
 * |factory /comms/gamma(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Gamma.cpp:92-102
Block *gammaFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return new Unary("Gamma", dtype, scalar, PCX_SPEC_GAMMA);
    throw InvalidArgumentException("gammaFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerGamma("/comms/gamma", &gammaFactory);

/***********************************************************************
 * |PothosDoc Log Gamma
 *
 * Evaluates the logarithm of the magnitude of the gamma function at every element of a stream on the GPU, which stays finite long
 * after the gamma function itself has overflowed.  Zero, the negative integers and both infinities give plus infinity.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output: float32 or float64.
 * |widget DTypeChooser(float=1)
 * |default "float64"
 * |preview disable
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
 * |factory /comms/lngamma(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Gamma.cpp:104-114
Block *lnGammaFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return new Unary("LnGamma", dtype, scalar, PCX_SPEC_LNGAMMA);
    throw InvalidArgumentException("lnGammaFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerLnGamma("/comms/lngamma", &lnGammaFactory);

/***********************************************************************
 * |PothosDoc Error Function
 *
 * Evaluates erf at every element of a stream on the GPU: the probability that a normal variable of variance one half falls
 * within the element's distance of its mean.  A zero keeps its sign, the infinities give plus and minus one.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output: float32 or float64.
 * |widget DTypeChooser(float=1)
 * |default "float64"
 * |preview disable
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
 * |factory /comms/erf(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// ErrorFunction.cpp:94-104
Block *erfFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return new Unary("Erf", dtype, scalar, PCX_SPEC_ERF);
    throw InvalidArgumentException("erfFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerErf("/comms/erf", &erfFactory);

/***********************************************************************
 * |PothosDoc Complementary Error Function
 *
 * Evaluates erfc, one less erf, at every element of a stream on the GPU without the cancellation that the subtraction suffers in
 * the tail.  Half of erfc of a level over the square root of two is the Q-function of a bit-error-rate curve.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output: float32 or float64.
 * |widget DTypeChooser(float=1)
 * |default "float64"
 * |preview disable
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
 * |factory /comms/erfc(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// ErrorFunction.cpp:106-116
Block *erfcFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return new Unary("Erfc", dtype, scalar, PCX_SPEC_ERFC);
    throw InvalidArgumentException("erfcFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerErfc("/comms/erfc", &erfcFactory);

/***********************************************************************
 * |PothosDoc Beta
 *
 * Evaluates the beta function of the elements of two streams, pair by pair, on the GPU, as the exponential of a sum of three
 * log-gamma values.  That expression is the one the C++ library computes, so a negative argument yields the magnitude of the
 * beta function and not its sign.
 *
 * |category /Math
 * |keywords euler integral gamma
 *
 * |param dtype[Data Type] Element type of both inputs and of the output: float32 or float64.
 * |widget DTypeChooser(float=1)
 * |default "float64"
 * |preview disable
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
 * |factory /comms/beta(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Beta.cpp:87-96
Block *betaFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return new Beta(dtype, scalar);
    throw InvalidArgumentException("betaFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerBeta("/comms/beta", &betaFactory);

/***********************************************************************
 * |PothosDoc Decompose Floats
 *
 * Takes every element of a stream apart on the GPU: the whole number towards zero goes to output port "int", what is left goes
 * to output port "frac".  Both parts carry the sign of the element and add up to it exactly.
 *
 * |category /Math
 * |keywords math fractional
 *
 * |param dtype[Data Type] Element type of the input and of both outputs: float32 or float64.
 * |widget DTypeChooser(float=1,dim=1)
 * |default "float64"
 * |preview disable
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
 * |factory /comms/modf(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// ModF.cpp:102-113
Block *modfFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return new ModF(dtype, scalar);
    throw InvalidArgumentException("modfFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerModF("/comms/modf", &modfFactory);

}  // namespace
