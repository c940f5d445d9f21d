// math_blocks.cpp -- the thirteenth module of this port, libpcx_math_blocks.so (with the runner ABI of include/pcx_blocks.h linked in):
// the real-valued function blocks of the reference's math/ directory.  In a PothosComms build they join the MathBlocks module
// (INTEGRATION.md).
//
//   /comms/exp exp2 exp10 expm1 expN      math/Exp.cpp:111-234
//   /comms/log log2 log10 log1p logN      math/Log.cpp:126-253
//   /comms/pow                            math/Pow.cpp:71-165
//   /comms/sqrt cbrt nth_root             math/Root.cpp:183-327
//   /comms/rsqrt                          math/RSqrt.cpp:42-110
//   /comms/sinc                           math/Sinc.cpp:74-121
//   /comms/sigmoid                        math/Sigmoid.cpp:60-107
//   /comms/trigonometric                  math/Trigonometric.cpp:463-555
//
// float32 and float64.  The reference also instantiates the exp, log, pow and root families for the eight integer types; those are
// not built (a last-place difference before the truncation becomes a difference of 1), and their factories refuse an
// integer dtype with the words the reference uses for a type it does not know.
//
// The maps are stateless calls of include/pcx.h (csrc/mathfn.hip): a block holds the function it is set to, its parameter and the
// device it runs on.  Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;

namespace {

using namespace pcxblk;     // parseElemType, check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_mathfn_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

// which scalars of a port buffer one work() maps.  REFERENCE QUIRK, reproduced: Exp::work (Exp.cpp:128-141) and Log::work
// (Log.cpp:143-156) hand their loop `elems`, not elems times the dimension -- on a stream of dimension d > 1 the first elems scalars of
// the buffer are mapped and elems elements (elems * d scalars) are consumed and produced.  Root::work (Root.cpp:199-213), Pow::work
// (Pow.cpp:105-118), RSqrt::work (RSqrt.cpp:56-70), Sinc::work (Sinc.cpp:86-104), Sigmoid::work (Sigmoid.cpp:72-90) and
// Trigonometric::work (Trigonometric.cpp:513-530) multiply by the dimension.
enum class Count { Elements, Scalars };

// what the blocks share: the function of pcx_math_fn they are set to, its parameter if it has one, one work()
template <typename T>
class FnBlock : public PortBlock {
public:
    FnBlock(const std::string &who, const DType &dtype, Count count) : PortBlock(who, kPortSlabBytes), _where(who + "::work()"), _count(count)
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(FnBlock, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(FnBlock, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(FnBlock, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(FnBlock, getPortSlabBytes));
    }
    void setDevice(const size_t device) { _device = checkedDevice(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t n = _count == Count::Scalars ? elems * inPort->dtype().dimension() : elems;
        const void *in = inPort->buffer().template as<const void *>();
        void *out = outPort->buffer().template as<void *>();
        constexpr int scalar = std::is_same<T, double>::value ? PCX_F64 : PCX_F32;
        OnDevice on(_device, _where.c_str());
        check(_withParam ? pcx_mathfn_param(scalar, _fn, &_param, in, out, n) : pcx_mathfn(scalar, _fn, in, out, n), _where);
        inPort->consume(elems);
        outPort->produce(elems);
    }

protected:
    void select(int fn) { _fn = fn; _withParam = false; }
    void select(int fn, T param) { _fn = fn; _param = param; _withParam = true; }

private:
    const std::string _where;
    const Count _count;
    int _fn = PCX_MATH_EXP;
    bool _withParam = false;
    T _param = T();
};

// a block of one fixed function
template <typename T>
class Fixed : public FnBlock<T> {
public:
    Fixed(const std::string &who, const DType &dtype, Count count, int fn) : FnBlock<T>(who, dtype, count) { this->select(fn); }
};

bool isFloat(const DType &dtype, int &scalar)
{
    bool cplx;
    return parseElemType(dtype, scalar, cplx) && !cplx && (scalar == PCX_F64 || scalar == PCX_F32);
}
Block *makeFixed(const std::string &who, const DType &dtype, int scalar, Count count, int fn)
{
    if (scalar == PCX_F64) return new Fixed<double>(who, dtype, count, fn);
    return new Fixed<float>(who, dtype, count, fn);
}

/***********************************************************************
 * |PothosDoc Exp
 *
 * Raises e to every element of a stream on the GPU.  A float32 element is widened, taken through the double-precision
 * exponential and rounded once, so it lies within one unit in the last place of the correctly rounded value.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/exp(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Exp.cpp:195-211
Block *expFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Exp", dtype, scalar, Count::Elements, PCX_MATH_EXP);
    throw InvalidArgumentException("expFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerExp("/comms/exp", &expFactory);

/***********************************************************************
 * |PothosDoc Exp2
 *
 * Raises 2 to every element of a stream on the GPU, for float32 through the double-precision function with one rounding.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/exp2(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Exp.cpp:212
Block *exp2Factory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Exp2", dtype, scalar, Count::Elements, PCX_MATH_EXP2);
    throw InvalidArgumentException("exp2Factory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerExp2("/comms/exp2", &exp2Factory);

/***********************************************************************
 * |PothosDoc Exp10
 *
 * Raises 10 to every element of a stream on the GPU: the way back from a level in decibels (after a division by 20) to an
 * amplitude.  For float32 through the double-precision function with one rounding.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/exp10(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Exp.cpp:213
Block *exp10Factory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Exp10", dtype, scalar, Count::Elements, PCX_MATH_EXP10);
    throw InvalidArgumentException("exp10Factory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerExp10("/comms/exp10", &exp10Factory);

/***********************************************************************
 * |PothosDoc Exp(n)-1
 *
 * Computes e to the element, less one, for every element of a stream on the GPU, without the cancellation the two separate
 * steps suffer next to zero.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/expm1(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Exp.cpp:214
Block *expm1Factory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Expm1", dtype, scalar, Count::Elements, PCX_MATH_EXPM1);
    throw InvalidArgumentException("expm1Factory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerExpm1("/comms/expm1", &expm1Factory);

/***********************************************************************
 * |PothosDoc Exp N
 *
 * Raises a chosen base to every element of a stream on the GPU.  The base 10 takes the path of the Exp10 block; every other base,
 * 2 among them, takes the general power function, as the reference's setter ends up doing.
 *
 * |category /Math
 * |setter setBase(base)
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
 * |preview disable
 *
 * |param base[Base] The number that is raised to the elements, converted to the element type.
 * |widget LineEdit()
 * |default 10
 * |preview enable
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
 * |factory /comms/expN(dtype,base)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class ExpN : public FnBlock<T> {
public:
    ExpN(const DType &dtype, T base) : FnBlock<T>("ExpN", dtype, Count::Elements)
    {
        this->registerCall(this, PCX_FCN_TUPLE(ExpN, base));
        this->registerCall(this, PCX_FCN_TUPLE(ExpN, setBase));
        this->registerProbe("base");
        this->registerSignal("baseChanged");
        this->setBase(base);
    }
    T base() const { return _base; }
    // Exp.cpp:171-181 (:176-178) reads `if (base == 2) exp2; if (base == 10) exp10; else generic`: the second statement's else overrides the
    // first, so base 2 runs the generic pow(base, x) and only base 10 leaves it
    void setBase(T base)
    {
        _base = base;
        if (_base == T(10)) this->select(PCX_MATH_EXP10);
        else this->select(PCX_MATH_EXPN, _base);
        this->emitSignal("baseChanged");
    }

private:
    T _base;
};
// Exp.cpp:216-234
Block *expNFactory(const DType &dtype, const pcxfw::Object &base)
{
    int scalar;
    if (isFloat(dtype, scalar)) {
        if (scalar == PCX_F64) return new ExpN<double>(dtype, base.convert<double>());
        return new ExpN<float>(dtype, base.convert<float>());
    }
    throw InvalidArgumentException("expNFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerExpN("/comms/expN", &expNFactory);

/***********************************************************************
 * |PothosDoc Log
 *
 * Takes the natural logarithm of every element of a stream on the GPU.  Zero gives minus infinity and a negative element a NaN.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/log(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Log.cpp:215-231
Block *logFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Log", dtype, scalar, Count::Elements, PCX_MATH_LOG);
    throw InvalidArgumentException("logFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerLog("/comms/log", &logFactory);

/***********************************************************************
 * |PothosDoc Log2
 *
 * Takes the logarithm to the base 2 of every element of a stream on the GPU.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/log2(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Log.cpp:232
Block *log2Factory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Log2", dtype, scalar, Count::Elements, PCX_MATH_LOG2);
    throw InvalidArgumentException("log2Factory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerLog2("/comms/log2", &log2Factory);

/***********************************************************************
 * |PothosDoc Log10
 *
 * Takes the logarithm to the base 10 of every element of a stream on the GPU.  Behind a magnitude and in front of a
 * multiplication by 20 it gives a level in decibels without the samples leaving device memory.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/log10(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Log.cpp:233
Block *log10Factory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Log10", dtype, scalar, Count::Elements, PCX_MATH_LOG10);
    throw InvalidArgumentException("log10Factory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerLog10("/comms/log10", &log10Factory);

/***********************************************************************
 * |PothosDoc Log(x+1)
 *
 * Takes the natural logarithm of one plus the element for every element of a stream on the GPU, accurate next to zero where
 * the sum would lose the element's low bits.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
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
 * |factory /comms/log1p(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Log.cpp:234
Block *log1pFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Log1p", dtype, scalar, Count::Elements, PCX_MATH_LOG1P);
    throw InvalidArgumentException("log1pFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerLog1p("/comms/log1p", &log1pFactory);

/***********************************************************************
 * |PothosDoc Log N
 *
 * Takes the logarithm to a chosen base of every element of a stream on the GPU.  The base 10 takes the path of the Log10 block;
 * every other base, 2 among them, is the quotient of two natural logarithms, as the reference's setter ends up doing.
 *
 * |category /Math
 * |setter setBase(base)
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float32"
 * |preview disable
 *
 * |param base[Base] The base of the logarithm, converted to the element type; it has to be positive.
 * |widget LineEdit()
 * |default 10
 * |preview enable
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
 * |factory /comms/logN(dtype,base)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class LogN : public FnBlock<T> {
public:
    LogN(const DType &dtype, T base) : FnBlock<T>("LogN", dtype, Count::Elements)
    {
        this->registerCall(this, PCX_FCN_TUPLE(LogN, base));
        this->registerCall(this, PCX_FCN_TUPLE(LogN, setBase));
        this->registerProbe("base");
        this->registerSignal("baseChanged");
        this->setBase(base);
    }
    T base() const { return _base; }
    // Log.cpp:186-201 (:196-198): the range check, then the same pair of statements as Exp.cpp's -- base 2 runs log(x) / log(base)
    void setBase(T base)
    {
        if (base <= 0) throw pcxfw::RangeException("LogN::setBase(" + std::to_string(base) + ")", "Log base must be > 0");
        _base = base;
        if (_base == T(10)) this->select(PCX_MATH_LOG10);
        else this->select(PCX_MATH_LOGN, _base);
        this->emitSignal("baseChanged");
    }

private:
    T _base;
};
// Log.cpp:236-254
Block *logNFactory(const DType &dtype, const pcxfw::Object &base)
{
    int scalar;
    if (isFloat(dtype, scalar)) {
        if (scalar == PCX_F64) return new LogN<double>(dtype, base.convert<double>());
        return new LogN<float>(dtype, base.convert<float>());
    }
    throw InvalidArgumentException("logNFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerLogN("/comms/logN", &logNFactory);

/***********************************************************************
 * |PothosDoc Pow
 *
 * Raises every element of a stream to one fixed exponent on the GPU, with the special cases of the C power function: a negative
 * element under a fractional exponent gives a NaN, any element under the exponent 0 gives 1.
 *
 * |category /Math
 * |keywords exponent
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(int=1,uint=1,float=1,dim=1)
 * |default "float64"
 * |preview disable
 *
 * |param exponent[Exponent] The power every element is raised to, converted to the element type.
 * |widget SpinBox()
 * |default 0
 * |preview enable
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
 * |factory /comms/pow(dtype,exponent)
 * |setter setExponent(exponent)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class Pow : public FnBlock<T> {
public:
    Pow(const DType &dtype, T exponent) : FnBlock<T>("Pow", dtype, Count::Scalars)
    {
        this->registerCall(this, PCX_FCN_TUPLE(Pow, exponent));
        this->registerCall(this, PCX_FCN_TUPLE(Pow, setExponent));
        this->registerProbe("exponent");
        this->registerSignal("exponentChanged");
        this->setExponent(exponent);
    }
    T exponent() const { return _exponent; }
    // Pow.cpp:97-103 (the validation of :125-132 concerns the signed integer types only)
    void setExponent(T exponent)
    {
        _exponent = exponent;
        this->select(PCX_MATH_POW, _exponent);
        this->emitSignal("exponentChanged");
    }

private:
    T _exponent;
};
// Pow.cpp:147-165
Block *powFactory(const DType &dtype, const pcxfw::Object &exponent)
{
    int scalar;
    if (isFloat(dtype, scalar)) {
        if (scalar == PCX_F64) return new Pow<double>(dtype, exponent.convert<double>());
        return new Pow<float>(dtype, exponent.convert<float>());
    }
    throw InvalidArgumentException("powFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerPow("/comms/pow", &powFactory);

/***********************************************************************
 * |PothosDoc Square Root
 *
 * Takes the square root of every element of a stream on the GPU, correctly rounded in both types: the result equals the
 * host's bit for bit.  A negative element gives a NaN, minus zero stays minus zero.
 *
 * |category /Math
 * |keywords sqrt
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
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
 * |factory /comms/sqrt(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Root.cpp:262-280
Block *makeSqrt(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Sqrt", dtype, scalar, Count::Scalars, PCX_MATH_SQRT);
    throw InvalidArgumentException("makeSqrt: unsupported type: " + dtype.toString());
}
pcxfw::BlockRegistry registerSqrt("/comms/sqrt", &makeSqrt);

/***********************************************************************
 * |PothosDoc Cube Root
 *
 * Takes the cube root of every element of a stream on the GPU; a negative element has a negative root.
 *
 * |category /Math
 * |keywords cbrt
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
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
 * |factory /comms/cbrt(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Root.cpp:282-300
Block *makeCbrt(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Cbrt", dtype, scalar, Count::Scalars, PCX_MATH_CBRT);
    throw InvalidArgumentException("makeCbrt: unsupported type: " + dtype.toString());
}
pcxfw::BlockRegistry registerCbrt("/comms/cbrt", &makeCbrt);

/***********************************************************************
 * |PothosDoc Nth Root
 *
 * Takes a chosen root of every element of a stream on the GPU, as the power 1 / N in double precision.  Where N is an odd
 * positive integer a negative element is mirrored and has a negative root; under every other N it gives a NaN.  The root 3 takes
 * the path of the Cube Root block; the root 2 takes the general power, as the reference's setter ends up doing, so minus zero
 * becomes plus zero and minus infinity plus infinity.
 *
 * |category /Math
 * |setter setRoot(root)
 *
 * |param dtype[Data Type] Element type of the input and of the output; float32 and float64 run on the GPU, an integer type is refused.
 * |widget DTypeChooser(float=1,int=1,uint=1,dim=1)
 * |default "float64"
 * |preview disable
 *
 * |param root[Root] Which root is taken, converted to the element type.
 * |widget SpinBox()
 * |default 1
 * |preview enable
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
 * |factory /comms/nth_root(dtype,root)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class NthRoot : public FnBlock<T> {
public:
    NthRoot(const DType &dtype, T root) : FnBlock<T>("NthRoot", dtype, Count::Scalars)
    {
        this->registerCall(this, PCX_FCN_TUPLE(NthRoot, root));
        this->registerCall(this, PCX_FCN_TUPLE(NthRoot, setRoot));
        this->registerProbe("root");
        this->registerSignal("rootChanged");
        this->setRoot(root);
    }
    T root() const { return _root; }
    // Root.cpp:242-252 (:247-249) reads `if (root == 2) sqrt; if (root == 3) cbrt; else nth root`: the second statement's else overrides the
    // first, so root 2 runs the generic pow(x, 1.0 / root) and only root 3 leaves it.  Which of the two generic expressions a root takes
    // (Root.cpp:161-165) is decided where the parameter is read, in pcx_mathfn_param.
    void setRoot(T root)
    {
        _root = root;
        if (_root == T(3)) this->select(PCX_MATH_CBRT);
        else this->select(PCX_MATH_NTH_ROOT, _root);
        this->emitSignal("rootChanged");
    }

private:
    T _root;
};
// Root.cpp:302-320
Block *makeNthRoot(const DType &dtype, const pcxfw::Object &root)
{
    int scalar;
    if (isFloat(dtype, scalar)) {
        if (scalar == PCX_F64) return new NthRoot<double>(dtype, root.convert<double>());
        return new NthRoot<float>(dtype, root.convert<float>());
    }
    throw InvalidArgumentException("makeNthRoot: unsupported type: " + dtype.toString());
}
pcxfw::BlockRegistry registerNthRoot("/comms/nth_root", &makeNthRoot);

/***********************************************************************
 * |PothosDoc Reciprocal Square Root
 *
 * Computes one over the square root of every element of a stream on the GPU.  On float64 that is a correctly rounded root and
 * a correctly rounded division.  On float32 it is the reference's fast approximation -- an integer subtraction on the bit
 * pattern and one refinement step in single precision, good to about three digits -- reproduced bit for bit.
 *
 * |category /Math
 *
 * |param dtype[Data Type] Element type of the input and of the output, float32 or float64.
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
 * |factory /comms/rsqrt(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// RSqrt.cpp:98-108
Block *makeRSqrt(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("RSqrt", dtype, scalar, Count::Scalars, PCX_MATH_RSQRT);
    throw InvalidArgumentException("Unsupported dtype: " + dtype.toString());
}
pcxfw::BlockRegistry registerRSqrt("/comms/rsqrt", &makeRSqrt);

/***********************************************************************
 * |PothosDoc Sinc
 *
 * Computes the unnormalised cardinal sine of every element of a stream on the GPU.  An element closer to zero than one millionth
 * gives exactly 1; every other element gives its sine divided by itself.
 *
 * |category /Math
 * |keywords math sin
 *
 * |param dtype[Data Type] Element type of the input and of the output, float32 or float64.
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
 * |factory /comms/sinc(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Sinc.cpp:113-121
Block *sincFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Sinc", dtype, scalar, Count::Scalars, PCX_MATH_SINC);
    throw InvalidArgumentException("sincFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerSinc("/comms/sinc", &sincFactory);

/***********************************************************************
 * |PothosDoc Sigmoid
 *
 * Computes the logistic function of every element of a stream on the GPU, the soft decision between 0 and 1.  A float32 element
 * far below zero gives the small true value where the reference's single-precision exponential overflows and returns 0.
 *
 * |category /Math
 * |keywords math sin
 *
 * |param dtype[Data Type] Element type of the input and of the output, float32 or float64.
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
 * |factory /comms/sigmoid(dtype)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// Sigmoid.cpp:99-107
Block *sigmoidFactory(const DType &dtype)
{
    int scalar;
    if (isFloat(dtype, scalar)) return makeFixed("Sigmoid", dtype, scalar, Count::Scalars, PCX_MATH_SIGMOID);
    throw InvalidArgumentException("sigmoidFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerSigmoid("/comms/sigmoid", &sigmoidFactory);

/***********************************************************************
 * |PothosDoc Trigonometric
 *
 * Applies one circular or hyperbolic function, or one of their inverses, to every element of a stream on the GPU.  The six
 * reciprocal functions (SEC, CSC, COT and their hyperbolic forms) are one over the function of the element; the six inverse
 * reciprocal functions (ASEC ... ACOTH) are the inverse function of one over the element.  Angles are in radians.
 *
 * |category /Math
 * |keywords cos sin tan sec csc cot
 *
 * |param dtype[Data Type] Element type of the input and of the output, float32 or float64.
 * |widget DTypeChooser(float=1,dim=1)
 * |default "float32"
 * |preview disable
 *
 * |param operation Which of the 24 functions every element goes through; it can be changed while the block runs.
 * |widget ComboBox(editable=false)
 * |default "COS"
 * |option [Cos] "COS"
 * |option [Sin] "SIN"
 * |option [Tan] "TAN"
 * |option [Sec] "SEC"
 * |option [Csc] "CSC"
 * |option [Cot] "COT"
 * |option [ArcCos] "ACOS"
 * |option [ArcSin] "ASIN"
 * |option [ArcTan] "ATAN"
 * |option [ArcSec] "ASEC"
 * |option [ArcCsc] "ACSC"
 * |option [ArcCot] "ACOT"
 * |option [CosH] "COSH"
 * |option [SinH] "SINH"
 * |option [TanH] "TANH"
 * |option [SecH] "SECH"
 * |option [CscH] "CSCH"
 * |option [CotH] "COTH"
 * |option [ArcCosH] "ACOSH"
 * |option [ArcSinH] "ASINH"
 * |option [ArcTanH] "ATANH"
 * |option [ArcSecH] "ASECH"
 * |option [ArcCscH] "ACSCH"
 * |option [ArcCotH] "ACOTH"
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
 * |factory /comms/trigonometric(dtype, operation)
 * |initializer setOperation(operation)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class Trigonometric : public FnBlock<T> {
public:
    Trigonometric(const DType &dtype, const std::string &operation) : FnBlock<T>("Trigonometric", dtype, Count::Scalars)
    {
        this->setOperation(operation);
        this->registerCall(this, PCX_FCN_TUPLE(Trigonometric, setOperation));
    }
    // Trigonometric.cpp:481-511; the codes of pcx_math_fn follow the order of the description's options
    void setOperation(const std::string &funcName)
    {
        static const char *const names[] = {"COS",  "SIN",  "TAN",  "SEC",  "CSC",  "COT",  "ACOS",  "ASIN",  "ATAN",  "ASEC",  "ACSC",  "ACOT",
                                            "COSH", "SINH", "TANH", "SECH", "CSCH", "COTH", "ACOSH", "ASINH", "ATANH", "ASECH", "ACSCH", "ACOTH"};
        for (int i = 0; i < 24; i++)
            if (funcName == names[i]) {
                this->select(PCX_MATH_COS + i);
                return;
            }
        throw InvalidArgumentException("Invalid operation", funcName);
    }
};
// Trigonometric.cpp:541-555
Block *makeTrigonometric(const DType &dtype, const std::string &operation)
{
    int scalar;
    if (isFloat(dtype, scalar)) {
        if (scalar == PCX_F64) return new Trigonometric<double>(dtype, operation);
        return new Trigonometric<float>(dtype, operation);
    }
    throw InvalidArgumentException("makeTrigonometric: unsupported type", dtype.name());
}
pcxfw::BlockRegistry registerTrigonometric("/comms/trigonometric", &makeTrigonometric);

}  // namespace
