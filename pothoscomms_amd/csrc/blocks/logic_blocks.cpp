// logic_blocks.cpp -- the twelfth module of this port, libpcx_logic_blocks.so (with the runner ABI of include/pcx_blocks.h linked in):
// the comparators and the arithmetic with a constant of the reference's math/ directory, the bitwise and byte-order blocks of its
// digital/ directory.  In a PothosComms build the first three classes below join the MathBlocks module and the other five the
// DigitalBlocks module.
//
//   /comms/comparator             math/Comparator.cpp:118-207
//   /comms/const_comparator       math/ConstComparator.cpp:133-251
//   /comms/const_arithmetic       math/ConstArithmetic.cpp:128-267
//   /comms/bitwise_unary          digital/Bitwise.cpp:117-153, :340-357
//   /comms/bitwise_binary         digital/Bitwise.cpp:155-193, :359-388
//   /comms/const_bitwise_binary   digital/Bitwise.cpp:195-253, :390-416
//   /comms/bitshift               digital/Bitwise.cpp:255-321, :418-440
//   /comms/byte_order             digital/ByteOrder.cpp:114-270 (the stream path; the bundled runtime has no messages, so the packet
//                                 path of :194-224 is not built)
//
// The maps are stateless calls of include/pcx.h (csrc/logic.hip): a block holds its settings and the device it runs on.
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <complex>
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

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_logic_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

// the element types of this module: parseElemType's six and the unsigned integers
bool parseLogicType(const DType &dt, int &scalar, bool &cplx)
{
    if (parseElemType(dt, scalar, cplx)) return true;
    std::string n = DType::fromDType(dt, 1).name();
    cplx = n.compare(0, 8, "complex_") == 0;
    if (cplx) n = n.substr(8);
    if (n == "uint64") scalar = PCX_U64;
    else if (n == "uint32") scalar = PCX_U32;
    else if (n == "uint16") scalar = PCX_U16;
    else if (n == "uint8") scalar = PCX_U8;
    else return false;
    return true;
}
bool isIntegerScalar(int scalar) { return scalar != PCX_F64 && scalar != PCX_F32; }
int comparisonCode(const std::string &op)
{
    return op == ">" ? PCX_CMP_GT : op == "<" ? PCX_CMP_LT : op == ">=" ? PCX_CMP_GE : op == "<=" ? PCX_CMP_LE : op == "==" ? PCX_CMP_EQ
           : op == "!=" ? PCX_CMP_NE : -1;
}
int bitwiseCode(const std::string &op) { return op == "AND" ? PCX_BIT_AND : op == "OR" ? PCX_BIT_OR : op == "XOR" ? PCX_BIT_XOR : -1; }
// the exception of digital/Bitwise.cpp:328-337
InvalidArgumentException bitwiseParamException(const DType &dtype, const std::string &operation)
{
    return InvalidArgumentException("DType: " + dtype.toString() + ", Operation: " + operation);
}

// what the eight blocks share beyond PortBlock: no handle, so a device change is a number
class LogicBlock : public PortBlock {
public:
    explicit LogicBlock(const std::string &who) : PortBlock(who, kPortSlabBytes) {}

protected:
    void moveTo(const size_t device) { _device = checkedDevice(device); }
};

/***********************************************************************
 * |PothosDoc Comparator
 *
 * Compares two streams element by element on the GPU and writes one byte per pair: 1 where the relation holds, 0 where it
 * does not.  The relation is the C++ operator of the element type, so a NaN on either side makes every relation but != false.
 * The bytes feed the blocks that work on bits and symbols without leaving device memory.
 *
 * |category /Math
 * |keywords math logic comparator
 *
 * |param dtype[Data Type] Element type of both inputs.
 * |widget DTypeChooser(float=1,int=1,dim=1)
 * |default "float64"
 * |preview disable
 *
 * |param comparator Which relation between input 0 and input 1 yields a 1.
 * |default ">"
 * |option [>] ">"
 * |option [<] "<"
 * |option [>=] ">="
 * |option [<=] "<="
 * |option [==] "=="
 * |option [!=] "!="
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
 * |factory /comms/comparator(dtype,comparator)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class Comparator : public LogicBlock {
public:
    Comparator(const DType &dtype, int scalar, int op) : LogicBlock("Comparator"), _scalar(scalar), _op(op)
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupInput(1, dtype, kDomain);
        Block::setupOutput(0, DType("int8"), kDomain);        // typeid(char), dimension 1 (Comparator.cpp:151)
        this->registerCall(this, PCX_FCN_TUPLE(Comparator, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(Comparator, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(Comparator, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(Comparator, getPortSlabBytes));
    }
    void setDevice(const size_t device) { moveTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (Comparator.cpp:154-175).  REFERENCE QUIRK, reproduced: the count handed to the loop is elems times the dimension of the
    // OUTPUT port, which is 1 -- with inputs of dimension d > 1 the first elems scalars of the buffers are compared, and elems
    // elements (elems * d scalars) are consumed.
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto in0 = this->input(0);
        auto in1 = this->input(1);
        auto outPort = this->output(0);
        OnDevice on(_device, "Comparator::work()");
        check(pcx_compare(_scalar, _op, in0->buffer().template as<const void *>(), in1->buffer().template as<const void *>(),
                          outPort->buffer().template as<void *>(), elems * outPort->dtype().dimension()),
              "Comparator::work()");
        in0->consume(elems);
        in1->consume(elems);
        outPort->produce(elems);
    }

private:
    const int _scalar, _op;
};

// Comparator.cpp:184-203: the six signed and float types
Block *comparatorFactory(const DType &dtype, const std::string &operation)
{
    int scalar;
    bool cplx;
    const int op = comparisonCode(operation);
    if (op >= 0 && parseElemType(dtype, scalar, cplx) && !cplx) return new Comparator(dtype, scalar, op);
    throw InvalidArgumentException("Comparator(" + dtype.toString() + ", " + operation + ")", "unsupported args");
}
pcxfw::BlockRegistry registerComparator("/comms/comparator", &comparatorFactory);

/***********************************************************************
 * |PothosDoc Const Comparator
 *
 * Compares every element of a stream with one fixed value on the GPU and writes one byte per element: 1 where the relation
 * holds, 0 where it does not.  With the relation > and the value 0 this is the hard decision that turns samples into bits.
 *
 * |category /Math
 * |keywords math logic comparator
 *
 * |param dtype[Data Type] Element type of the input.
 * |widget DTypeChooser(float=1,int=1,dim=1)
 * |default "float64"
 * |preview disable
 *
 * |param comparator Which relation between an input element and the value yields a 1.
 * |default ">"
 * |option [>] ">"
 * |option [<] "<"
 * |option [>=] ">="
 * |option [<=] "<="
 * |option [==] "=="
 * |option [!=] "!="
 *
 * |param constant[Constant] The value on the right of the relation, converted to the element type.
 * |widget LineEdit()
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
 * |factory /comms/const_comparator(dtype,comparator)
 * |setter setConstant(constant)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename Type>
class ConstComparator : public LogicBlock {
public:
    ConstComparator(const DType &dtype, int scalar, int op) : LogicBlock("ConstComparator"), _scalar(scalar), _op(op), _constant(0)
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, DType("int8"), kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(ConstComparator, constant));
        this->registerCall(this, PCX_FCN_TUPLE(ConstComparator, setConstant));
        this->registerCall(this, PCX_FCN_TUPLE(ConstComparator, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(ConstComparator, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(ConstComparator, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(ConstComparator, getPortSlabBytes));
        this->registerProbe("constant");
        this->registerSignal("constantChanged");
    }
    Type constant() const { return _constant; }
    void setConstant(Type constant)
    {
        _constant = constant;
        this->emitSignal("constantChanged");        // (without the value: ConstComparator.cpp:193)
    }
    void setDevice(const size_t device) { moveTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (ConstComparator.cpp:196-215), with the quirk of Comparator::work: the output port's dimension counts the scalars
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        OnDevice on(_device, "ConstComparator::work()");
        check(pcx_compare_const(_scalar, _op, inPort->buffer().template as<const void *>(), &_constant, outPort->buffer().template as<void *>(),
                                elems * outPort->dtype().dimension()),
              "ConstComparator::work()");
        inPort->consume(elems);
        outPort->produce(elems);
    }

private:
    const int _scalar, _op;
    Type _constant;
};

// ConstComparator.cpp:224-247: the ten real element types
Block *constComparatorFactory(const DType &dtype, const std::string &operation)
{
    int scalar;
    bool cplx;
    const int op = comparisonCode(operation);
    if (op >= 0 && parseLogicType(dtype, scalar, cplx) && !cplx) {
        switch (scalar) {
        case PCX_F64: return new ConstComparator<double>(dtype, scalar, op);
        case PCX_F32: return new ConstComparator<float>(dtype, scalar, op);
        case PCX_I64: return new ConstComparator<int64_t>(dtype, scalar, op);
        case PCX_I32: return new ConstComparator<int32_t>(dtype, scalar, op);
        case PCX_I16: return new ConstComparator<int16_t>(dtype, scalar, op);
        case PCX_I8: return new ConstComparator<int8_t>(dtype, scalar, op);
        case PCX_U64: return new ConstComparator<uint64_t>(dtype, scalar, op);
        case PCX_U32: return new ConstComparator<uint32_t>(dtype, scalar, op);
        case PCX_U16: return new ConstComparator<uint16_t>(dtype, scalar, op);
        case PCX_U8: return new ConstComparator<uint8_t>(dtype, scalar, op);
        }
    }
    throw InvalidArgumentException("Comparator(" + dtype.toString() + ", " + operation + ")", "unsupported args");
}
pcxfw::BlockRegistry registerConstComparator("/comms/const_comparator", &constComparatorFactory);

/***********************************************************************
 * |PothosDoc Const Arithmetic
 *
 * Adds, subtracts, multiplies or divides every element of a stream and one fixed value on the GPU: the offset and the gain of a
 * flowgraph.  The operators are those of the arithmetic block, real or complex, with the value on the side the operation names.
 * An integer division by zero gives 0.
 *
 * |category /Math
 * |keywords math arithmetic add subtract multiply divide
 *
 * |param dtype[Data Type] Element type of the input, of the output and of the value.
 * |widget DTypeChooser(int=1,uint1=1,float=1,cint=1,cuint=1,cfloat=1,dim=1)
 * |default "float32"
 * |preview disable
 *
 * |param operation Which operation joins an element X and the value K.
 * |widget ComboBox(editable=false)
 * |default "X+K"
 * |option [X + K] "X+K"
 * |option [X - K] "X-K"
 * |option [K - X] "K-X"
 * |option [X * K] "X*K"
 * |option [X / K] "X/K"
 * |option [K / X] "K/X"
 * |preview enable
 *
 * |param constant[Constant] The value K, converted to the element type.
 * |widget LineEdit()
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
 * |factory /comms/const_arithmetic(dtype,operation,constant)
 * |setter setConstant(constant)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class ConstArithmetic : public LogicBlock {
public:
    ConstArithmetic(const DType &dtype, int scalar, bool cplx, int op, const T &constant)
        : LogicBlock("ConstArithmetic"), _scalar(scalar), _cplx(cplx), _op(op), _constant()
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(ConstArithmetic, constant));
        this->registerCall(this, PCX_FCN_TUPLE(ConstArithmetic, setConstant));
        this->registerCall(this, PCX_FCN_TUPLE(ConstArithmetic, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(ConstArithmetic, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(ConstArithmetic, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(ConstArithmetic, getPortSlabBytes));
        this->registerProbe("constant");
        this->registerSignal("constantChanged");
        this->setConstant(constant);
    }
    T constant() const { return _constant; }
    void setConstant(const T &constant)
    {
        _constant = constant;
        this->emitSignal("constantChanged", constant);
    }
    void setDevice(const size_t device) { moveTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (ConstArithmetic.cpp:200-219)
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        OnDevice on(_device, "ConstArithmetic::work()");
        // (a std::complex<U> is two U: the element the C ABI takes)
        check(pcx_arith_const(_scalar, _cplx ? 1 : 0, _op, inPort->buffer().template as<const void *>(), &_constant,
                              outPort->buffer().template as<void *>(), elems * inPort->dtype().dimension()),
              "ConstArithmetic::work()");
        inPort->consume(elems);
        outPort->produce(elems);
    }

private:
    const int _scalar;
    const bool _cplx;
    const int _op;
    T _constant;
};

template <typename U>
Block *makeConstArithmeticOf(const DType &dtype, int scalar, bool cplx, int op, const pcxfw::Object &constant)
{
    if (cplx) return new ConstArithmetic<std::complex<U>>(dtype, scalar, true, op, constant.convert<std::complex<U>>());
    return new ConstArithmetic<U>(dtype, scalar, false, op, constant.convert<U>());
}
// ConstArithmetic.cpp:228-263: the ten scalars, real and complex
Block *makeConstArithmetic(const DType &dtype, const std::string &operation, const pcxfw::Object &constant)
{
    int scalar;
    bool cplx;
    const int op = operation == "X+K" ? PCX_ARITHK_X_ADD_K : operation == "X-K" ? PCX_ARITHK_X_SUB_K : operation == "K-X" ? PCX_ARITHK_K_SUB_X
                   : operation == "X*K" ? PCX_ARITHK_X_MUL_K : operation == "X/K" ? PCX_ARITHK_X_DIV_K : operation == "K/X" ? PCX_ARITHK_K_DIV_X : -1;
    if (op >= 0 && parseLogicType(dtype, scalar, cplx)) {
        switch (scalar) {
        case PCX_F64: return makeConstArithmeticOf<double>(dtype, scalar, cplx, op, constant);
        case PCX_F32: return makeConstArithmeticOf<float>(dtype, scalar, cplx, op, constant);
        case PCX_I64: return makeConstArithmeticOf<int64_t>(dtype, scalar, cplx, op, constant);
        case PCX_I32: return makeConstArithmeticOf<int32_t>(dtype, scalar, cplx, op, constant);
        case PCX_I16: return makeConstArithmeticOf<int16_t>(dtype, scalar, cplx, op, constant);
        case PCX_I8: return makeConstArithmeticOf<int8_t>(dtype, scalar, cplx, op, constant);
        case PCX_U64: return makeConstArithmeticOf<uint64_t>(dtype, scalar, cplx, op, constant);
        case PCX_U32: return makeConstArithmeticOf<uint32_t>(dtype, scalar, cplx, op, constant);
        case PCX_U16: return makeConstArithmeticOf<uint16_t>(dtype, scalar, cplx, op, constant);
        case PCX_U8: return makeConstArithmeticOf<uint8_t>(dtype, scalar, cplx, op, constant);
        }
    }
    throw InvalidArgumentException("makeConstArithmetic(" + dtype.toString() + ", operation=" + operation + ")", "unsupported args");
}
pcxfw::BlockRegistry registerConstArithmetic("/comms/const_arithmetic", &makeConstArithmetic);

/***********************************************************************
 * |PothosDoc Bitwise Unary Operation
 *
 * Inverts every bit of an integer stream on the GPU.
 *
 * |category /Digital
 * |keywords not
 *
 * |param dtype[Data Type] Integer element type of the input and of the output.
 * |widget DTypeChooser(int=1,uint=1,dim=1)
 * |default "uint64"
 * |preview disable
 *
 * |param operation Which operation every element goes through; there is one.
 * |default "NOT"
 * |option [Not] "NOT"
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
 * |factory /comms/bitwise_unary(dtype,operation)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
/***********************************************************************
 * |PothosDoc Bitwise Binary Operation
 *
 * Joins the integer streams of two or more input ports bit by bit on the GPU.  However many ports there are, every input is read
 * once and the output written once.
 *
 * |category /Digital
 * |keywords and not xor
 *
 * |param dtype[Data Type] Integer element type of every input and of the output.
 * |widget DTypeChooser(int=1,uint=1,dim=1)
 * |default "uint64"
 * |preview disable
 *
 * |param operation Which operation folds the inputs into the output.
 * |default "AND"
 * |option [And] "AND"
 * |option [Or] "OR"
 * |option [XOr] "XOR"
 * |preview enable
 *
 * |param numChannels[Num Channels] How many input ports the block has.
 * |widget SpinBox(minimum=2)
 * |default 2
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
 * |factory /comms/bitwise_binary(dtype,operation,numChannels)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
// one class for the two: NOT of one port, or a fold over `nchans` ports (Bitwise.cpp:117-193)
class BitwiseArray : public LogicBlock {
public:
    BitwiseArray(const DType &dtype, int scalar, int op, size_t nchans) : LogicBlock(op == PCX_BIT_NOT ? "BitwiseUnaryArray" : "BitwiseBinaryArray"), _scalar(scalar), _op(op)
    {
        for (size_t chan = 0; chan < nchans; chan++) Block::setupInput(chan, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseArray, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseArray, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseArray, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseArray, getPortSlabBytes));
    }
    void setDevice(const size_t device) { moveTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (Bitwise.cpp:134-148, :171-188)
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto outPort = this->output(0);
        _ins.clear();
        for (auto *inPort : this->inputs()) _ins.push_back(inPort->buffer().template as<const void *>());
        OnDevice on(_device, "Bitwise::work()");
        check(pcx_bitwise(_scalar, _op, _ins.data(), _ins.size(), outPort->buffer().template as<void *>(), elems * outPort->dtype().dimension()), _who + "::work()");
        for (auto *inPort : this->inputs()) inPort->consume(elems);
        outPort->produce(elems);
    }

private:
    const int _scalar, _op;
    std::vector<const void *> _ins;
};

Block *makeBitwiseUnaryArray(const DType &dtype, const std::string &operation)
{
    int scalar;
    bool cplx;
    if (operation == "NOT" && parseLogicType(dtype, scalar, cplx) && !cplx && isIntegerScalar(scalar)) return new BitwiseArray(dtype, scalar, PCX_BIT_NOT, 1);
    throw bitwiseParamException(dtype, operation);
}
Block *makeBitwiseBinaryArray(const DType &dtype, const std::string &operation, size_t numChannels)
{
    int scalar;
    bool cplx;
    const int op = bitwiseCode(operation);
    // (fewer than two channels: the fold has nothing to fold, which the C ABI refuses; the reference's constructor takes any count)
    if (numChannels < 2)
        throw InvalidArgumentException("makeBitwiseBinaryArray(" + dtype.toString() + ", " + operation + ", numChannels=" + std::to_string(numChannels) + ")",
                                       "numChannels must be 2 or more");
    if (op >= 0 && parseLogicType(dtype, scalar, cplx) && !cplx && isIntegerScalar(scalar)) return new BitwiseArray(dtype, scalar, op, numChannels);
    throw bitwiseParamException(dtype, operation);
}
pcxfw::BlockRegistry registerBitwiseUnaryArray("/comms/bitwise_unary", &makeBitwiseUnaryArray);
pcxfw::BlockRegistry registerBitwiseBinaryArray("/comms/bitwise_binary", &makeBitwiseBinaryArray);

/***********************************************************************
 * |PothosDoc Bitwise Binary Const Operation
 *
 * Joins every element of an integer stream with one fixed value bit by bit on the GPU: a mask with AND, forced bits with OR, a
 * whitening pattern with XOR.
 *
 * |category /Digital
 * |keywords and not xor
 *
 * |param dtype[Data Type] Integer element type of the input, of the output and of the value.
 * |widget DTypeChooser(int=1,uint=1,dim=1)
 * |default "uint64"
 * |preview disable
 *
 * |param constant[Constant] The value every element is joined with, converted to the element type.
 * |widget SpinBox()
 * |default 0
 * |preview enable
 *
 * |param operation Which operation joins an element and the value.
 * |default "AND"
 * |option [And] "AND"
 * |option [Or] "OR"
 * |option [XOr] "XOR"
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
 * |factory /comms/const_bitwise_binary(dtype,constant,operation)
 * |setter setConstant(constant)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename Type>
class BitwiseBinaryConst : public LogicBlock {
public:
    BitwiseBinaryConst(const DType &dtype, int scalar, int op, const Type &constant) : LogicBlock("BitwiseBinaryConst"), _scalar(scalar), _op(op), _constant(0)
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseBinaryConst, constant));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseBinaryConst, setConstant));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseBinaryConst, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseBinaryConst, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseBinaryConst, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(BitwiseBinaryConst, getPortSlabBytes));
        this->registerProbe("constant");
        this->registerSignal("constantChanged");
        this->setConstant(constant);
    }
    Type constant() const { return _constant; }
    void setConstant(const Type &constant)
    {
        _constant = constant;
        this->emitSignal("constantChanged", constant);
    }
    void setDevice(const size_t device) { moveTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (Bitwise.cpp:234-248)
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        OnDevice on(_device, "BitwiseBinaryConst::work()");
        check(pcx_bitwise_const(_scalar, _op, inPort->buffer().template as<const void *>(), &_constant, outPort->buffer().template as<void *>(),
                                elems * outPort->dtype().dimension()),
              "BitwiseBinaryConst::work()");
        inPort->consume(elems);
        outPort->produce(elems);
    }

private:
    const int _scalar, _op;
    Type _constant;
};

Block *makeBitwiseBinaryConst(const DType &dtype, const pcxfw::Object &constant, const std::string &operation)
{
    int scalar;
    bool cplx;
    const int op = bitwiseCode(operation);
    if (op >= 0 && parseLogicType(dtype, scalar, cplx) && !cplx) {
        switch (scalar) {
        case PCX_I64: return new BitwiseBinaryConst<int64_t>(dtype, scalar, op, constant.convert<int64_t>());
        case PCX_I32: return new BitwiseBinaryConst<int32_t>(dtype, scalar, op, constant.convert<int32_t>());
        case PCX_I16: return new BitwiseBinaryConst<int16_t>(dtype, scalar, op, constant.convert<int16_t>());
        case PCX_I8: return new BitwiseBinaryConst<int8_t>(dtype, scalar, op, constant.convert<int8_t>());
        case PCX_U64: return new BitwiseBinaryConst<uint64_t>(dtype, scalar, op, constant.convert<uint64_t>());
        case PCX_U32: return new BitwiseBinaryConst<uint32_t>(dtype, scalar, op, constant.convert<uint32_t>());
        case PCX_U16: return new BitwiseBinaryConst<uint16_t>(dtype, scalar, op, constant.convert<uint16_t>());
        case PCX_U8: return new BitwiseBinaryConst<uint8_t>(dtype, scalar, op, constant.convert<uint8_t>());
        }
    }
    throw bitwiseParamException(dtype, operation);
}
pcxfw::BlockRegistry registerBitwiseBinaryConst("/comms/const_bitwise_binary", &makeBitwiseBinaryConst);

/***********************************************************************
 * |PothosDoc Bit Shift
 *
 * Moves the bits of every element of an integer stream to the left or to the right on the GPU.  A left shift drops what leaves
 * the element at the top; a right shift of a signed type repeats the sign bit, of an unsigned type fills with zeros.
 *
 * |category /Digital
 * |keywords left right
 *
 * |param dtype[Data Type] Integer element type of the input and of the output.
 * |widget DTypeChooser(int=1,uint=1,dim=1)
 * |default "uint64"
 * |preview disable
 *
 * |param operation In which direction the bits move.
 * |default "LEFTSHIFT"
 * |option [Left Shift] "LEFTSHIFT"
 * |option [Right Shift] "RIGHTSHIFT"
 * |preview enable
 *
 * |param shiftSize[Shift Size] By how many places the bits move, fewer than the element has bits.
 * |widget SpinBox(minimum=0)
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
 * |factory /comms/bitshift(dtype,operation,shiftSize)
 * |setter setShiftSize(shiftSize)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class BitShift : public LogicBlock {
public:
    BitShift(const DType &dtype, int scalar, bool leftShift, size_t shiftSize) : LogicBlock("BitShift"), _scalar(scalar), _bits(8 * DType::fromDType(dtype, 1).size()), _typeName(DType::fromDType(dtype, 1).toString()), _leftShift(leftShift), _shiftSize(0)
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(BitShift, shiftSize));
        this->registerCall(this, PCX_FCN_TUPLE(BitShift, setShiftSize));
        this->registerCall(this, PCX_FCN_TUPLE(BitShift, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(BitShift, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(BitShift, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(BitShift, getPortSlabBytes));
        this->registerProbe("shiftSize");
        this->registerSignal("shiftSizeChanged");
        this->setShiftSize(shiftSize);      // validates, and emits the signal (Bitwise.cpp:275-276)
    }
    size_t shiftSize() const { return _shiftSize; }
    // Bitwise.cpp:287-300
    void setShiftSize(size_t shiftSize)
    {
        if (shiftSize >= _bits)
            throw pcxfw::RangeException("BitShift::setShiftSize(" + std::to_string(shiftSize) + ")",
                                        "Shift size cannot be >= the number of bits (" + std::to_string(_bits) + ") in the type (" + _typeName + ")");
        _shiftSize = shiftSize;
        this->emitSignal("shiftSizeChanged", _shiftSize);
    }
    void setDevice(const size_t device) { moveTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (Bitwise.cpp:302-316)
    void work()
    {
        const size_t elems = this->workInfo().minElements;
        if (elems == 0) return;
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        OnDevice on(_device, "BitShift::work()");
        check(pcx_bitshift(_scalar, _leftShift ? 1 : 0, inPort->buffer().template as<const void *>(), _shiftSize, outPort->buffer().template as<void *>(),
                           elems * outPort->dtype().dimension()),
              "BitShift::work()");
        inPort->consume(elems);
        outPort->produce(elems);
    }

private:
    const int _scalar;
    const size_t _bits;
    const std::string _typeName;
    const bool _leftShift;
    size_t _shiftSize;
};

Block *makeBitShift(const DType &dtype, const std::string &operation, size_t shiftSize)
{
    int scalar;
    bool cplx;
    if ((operation == "LEFTSHIFT" || operation == "RIGHTSHIFT") && parseLogicType(dtype, scalar, cplx) && !cplx && isIntegerScalar(scalar))
        return new BitShift(dtype, scalar, operation == "LEFTSHIFT", shiftSize);
    throw bitwiseParamException(dtype, operation);
}
pcxfw::BlockRegistry registerBitShift("/comms/bitshift", &makeBitShift);

/***********************************************************************
 * |PothosDoc Byte Order
 *
 * Puts the bytes of every scalar of a stream into the chosen order on the GPU: the step between a payload as the network carries
 * it and the numbers the host computes with.  The two parts of a complex element are reversed each on its own.
 *
 * |category /Digital
 * |keywords bytes big little host network endian
 *
 * |param dtype[Data Type] Element type of the input and of the output, with scalars of 2, 4 or 8 bytes.
 * |widget DTypeChooser(int=1,uint=1,float=1,cint=1,cuint=1,cfloat=1,dim=1)
 * |default "uint64"
 * |preview disable
 *
 * |param byteOrder[Byte Order] Which order the output has, seen from this little-endian host.
 * |widget ComboBox(editable=false)
 * <ul>
 * <li><b>Swap Order</b> reverses every scalar whatever order it arrived in</li>
 * <li><b>Big Endian</b> reverses, since the host is little-endian</li>
 * <li><b>Little Endian</b> copies</li>
 * <li><b>Network to Host</b> reverses a big-endian stream into host numbers</li>
 * <li><b>Host to Network</b> reverses host numbers into a big-endian stream</li>
 * </ul>
 * |option [Swap Order] "Swap Order"
 * |option [Big Endian] "Big Endian"
 * |option [Little Endian] "Little Endian"
 * |option [Network to Host] "Network to Host"
 * |option [Host to Network] "Host to Network"
 * |default "Swap Order"
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
 * |factory /comms/byte_order(dtype)
 * |setter setByteOrder(byteOrder)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class ByteOrder : public LogicBlock {
public:
    ByteOrder(const DType &dtype, int width, int scalarsPerElement) : LogicBlock("ByteOrder"), _width(width), _per(scalarsPerElement), _order("Swap Order")
    {
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(ByteOrder, setByteOrder));
        this->registerCall(this, PCX_FCN_TUPLE(ByteOrder, getByteOrder));
        this->registerCall(this, PCX_FCN_TUPLE(ByteOrder, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(ByteOrder, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(ByteOrder, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(ByteOrder, getPortSlabBytes));
    }
    std::string getByteOrder() const { return _order; }
    // ByteOrder.cpp:180-192
    void setByteOrder(const std::string &order)
    {
        if (order != "Swap Order" && order != "Big Endian" && order != "Little Endian" && order != "Network to Host" && order != "Host to Network")
            throw InvalidArgumentException("Invalid byte order", order);
        _order = order;
    }
    void setDevice(const size_t device) { moveTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // work (ByteOrder.cpp:226-240: the stream path).  On this little-endian host every order but "Little Endian" reverses; that one
    // copies, with the same kernel shape: a byte-wise XOR with 0
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t numElements = std::min(inPort->elements(), outPort->elements());
        if (numElements == 0) return;
        const size_t scalars = numElements * inPort->dtype().dimension() * (size_t)_per;
        const void *in = inPort->buffer().template as<const void *>();
        void *out = outPort->buffer().template as<void *>();
        OnDevice on(_device, "ByteOrder::work()");
        if (_order == "Little Endian") {
            const unsigned char zero = 0;
            check(pcx_bitwise_const(PCX_U8, PCX_BIT_XOR, in, &zero, out, scalars * (size_t)_width), "ByteOrder::work()");
        } else {
            check(pcx_byteswap(_width, in, out, scalars), "ByteOrder::work()");
        }
        inPort->consume(numElements);
        outPort->produce(numElements);
    }

private:
    const int _width, _per;
    std::string _order;
};

// ByteOrder.cpp:242-263: the 16, 32 and 64-bit integers, float32, float64 and their complex forms
Block *makeByteOrder(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseLogicType(dtype, scalar, cplx) && scalar != PCX_I8 && scalar != PCX_U8)
        return new ByteOrder(dtype, (int)DType::fromDType(dtype, 1).size() / (cplx ? 2 : 1), cplx ? 2 : 1);
    throw InvalidArgumentException("Unsupported or invalid type", dtype.name());
}
pcxfw::BlockRegistry registerByteOrder("/comms/byte_order", &makeByteOrder);

}  // namespace
