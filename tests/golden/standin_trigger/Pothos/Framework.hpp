// Stand-in for <Pothos/Framework.hpp>: test infrastructure of this project, written new, not PothosCore.
//
// tests/golden/make_trigger_golden.py compiles a driver of its own against this header.  The driver includes utility/WaveTrigger.cpp of
// the reference BY PATH and runs its work() call after call.  The header holds exactly what that file uses, with bodies that RECORD:
// an input port hands out the buffer, the labels and the messages the driver planted and counts what is consumed and reserved; an
// output port collects what is posted.  As in Pothos, a port set up without a type counts in bytes, its buffers carry the type they
// were planted with, and a chunk, a packet or an object that was moved from is empty.  The two other stand-ins (tests/golden/standin,
// standin_sync) stay as they are; nothing here is shipped and nothing of the product includes it.
#pragma once
#include <complex>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <utility>
#include <vector>

#define POTHOS_FCN_TUPLE(c, m) #m, &c::m

namespace Pothos {

struct Exception : std::runtime_error {
    Exception(const std::string &where, const std::string &what) : std::runtime_error(where + ": " + what) {}
};
struct InvalidArgumentException : Exception {
    InvalidArgumentException(const std::string &where, const std::string &what) : Exception(where, what) {}
};

//! an element type by name ("int16", "complex_float32", ...); no name: unspecified, one byte per element
class DType {
public:
    DType() : _bytes(1) {}
    DType(const std::string &name) : _name(name), _bytes(bytesOf(name)) {}
    DType(const std::type_info &t) : _name(t == typeid(float) ? "float32" : "complex_float32"), _bytes(t == typeid(float) ? 4 : 8) {}
    size_t size() const { return _bytes; }
    bool isComplex() const { return _name.compare(0, 8, "complex_") == 0; }
    explicit operator bool() const { return !_name.empty(); }
    const std::string &name() const { return _name; }
    //! the scalar type's name
    std::string scalar() const { return isComplex() ? _name.substr(8) : _name; }

private:
    static size_t bytesOf(const std::string &name)
    {
        const bool cplx = name.compare(0, 8, "complex_") == 0;
        const std::string s = cplx ? name.substr(8) : name;
        const size_t b = s == "float64" || s == "int64" || s == "uint64" ? 8 : s == "float32" || s == "int32" || s == "uint32" ? 4 : s == "int16" || s == "uint16" ? 2 : 1;
        return cplx ? 2 * b : b;
    }
    std::string _name;
    size_t _bytes;
};

//! memory with a type: a view of the driver's stream, or storage of its own; copies share the storage
class BufferChunk {
public:
    size_t address, length;
    DType dtype;
    BufferChunk() : address(0), length(0) {}
    BufferChunk(const DType &dt, size_t numElems) : length(numElems * dt.size()), dtype(dt), _own(new std::vector<char>(length ? length : 1))
    {
        address = reinterpret_cast<size_t>(_own->data());
    }
    BufferChunk(const BufferChunk &) = default;
    BufferChunk &operator=(const BufferChunk &) = default;
    BufferChunk(BufferChunk &&o) : address(o.address), length(o.length), dtype(o.dtype), _own(std::move(o._own)) { o.address = o.length = 0; o.dtype = DType(); }
    BufferChunk &operator=(BufferChunk &&o)
    {
        address = o.address; length = o.length; dtype = o.dtype; _own = std::move(o._own);
        o.address = o.length = 0; o.dtype = DType();
        return *this;
    }
    static BufferChunk view(const void *p, size_t bytes, const DType &dt)
    {
        BufferChunk b;
        b.address = reinterpret_cast<size_t>(p);
        b.length = bytes;
        b.dtype = dt;
        return b;
    }
    size_t elements() const { return length / dtype.size(); }
    size_t getEnd() const { return address + length; }
    explicit operator bool() const { return address != 0; }
    template <typename T> T as() const { return reinterpret_cast<T>(address); }
    //! the elements as float, or as std::complex<float>: a static_cast per component
    BufferChunk convert(const DType &to) const
    {
        const size_t n = elements(), comps = dtype.isComplex() ? 2 : 1;
        BufferChunk out(to, n);
        float *y = out.as<float *>();
        const std::string s = dtype.scalar();
        const char *x = as<const char *>();
        for (size_t i = 0; i < n * comps; i++) {
            if (s == "float64") y[i] = component<double>(x, i);
            else if (s == "float32") y[i] = component<float>(x, i);
            else if (s == "int64") y[i] = component<int64_t>(x, i);
            else if (s == "int32") y[i] = component<int32_t>(x, i);
            else if (s == "int16") y[i] = component<int16_t>(x, i);
            else if (s == "int8") y[i] = component<int8_t>(x, i);
            else if (s == "uint64") y[i] = component<uint64_t>(x, i);
            else if (s == "uint32") y[i] = component<uint32_t>(x, i);
            else if (s == "uint16") y[i] = component<uint16_t>(x, i);
            else y[i] = component<uint8_t>(x, i);
        }
        return out;
    }

private:
    template <typename T> static float component(const char *x, size_t i)
    {
        T v;
        std::memcpy(&v, x + i * sizeof(T), sizeof(T));
        return static_cast<float>(v);
    }
    std::shared_ptr<std::vector<char>> _own;
};

//! any value by copy; empty after a move
class Object {
public:
    Object() : _t(&typeid(void)) {}
    Object(const Object &) = default;
    Object &operator=(const Object &) = default;
    Object(Object &&o) : _t(o._t), _p(std::move(o._p)) { o._t = &typeid(void); }
    Object &operator=(Object &&o)
    {
        _t = o._t; _p = std::move(o._p);
        o._t = &typeid(void);
        return *this;
    }
    template <typename T, typename D = typename std::decay<T>::type, typename = typename std::enable_if<!std::is_same<D, Object>::value>::type>
    Object(T &&v) : _t(&typeid(D)), _p(std::make_shared<D>(std::forward<T>(v))) {}
    const std::type_info &type() const { return *_t; }
    template <typename T> const T &extract() const { return *static_cast<const T *>(_p.get()); }

private:
    const std::type_info *_t;
    std::shared_ptr<void> _p;
};

struct Label {
    Label() : index(0), width(1) {}
    Label(const std::string &id_, const Object &data_, unsigned long long index_, size_t width_ = 1) : id(id_), data(data_), index(index_), width(width_) {}
    Label &adjust(size_t mult, size_t div)
    {
        index *= mult; width *= mult;
        index /= div; width /= div;
        return *this;
    }
    Label toAdjusted(size_t mult, size_t div) const
    {
        Label l = *this;
        return l.adjust(mult, div);
    }
    std::string id;
    Object data;
    unsigned long long index;
    size_t width;
};

struct Packet {
    BufferChunk payload;
    std::map<std::string, Object> metadata;
    std::vector<Label> labels;
};

class InputPort {
public:
    InputPort(int index) : consumed(0), reserve(0), reserveSet(false), _index(index) {}
    int index() const { return _index; }
    std::string name() const { return std::to_string(_index); }
    const BufferChunk &buffer() const { return buf; }
    BufferChunk takeBuffer() const { return buf; }
    size_t elements() const { return buf.length; }             // the port has no type: bytes
    const std::vector<Label> &labels() const { return labs; }
    void consume(size_t n) { consumed += n; }
    void setReserve(size_t n) { reserve = n; reserveSet = true; }
    bool hasMessage() const { return !msgs.empty(); }
    Object popMessage()
    {
        Object m = msgs.front();
        msgs.erase(msgs.begin());
        return m;
    }
    // the driver's side
    BufferChunk buf;
    std::vector<Label> labs;
    std::vector<Object> msgs;
    size_t consumed, reserve;
    bool reserveSet;

private:
    int _index;
};

class OutputPort {
public:
    template <typename T> void postMessage(T &&m) { posted.push_back(Object(std::forward<T>(m))); }
    // the driver's side
    std::vector<Object> posted;
};

struct BufferManager {
    typedef std::shared_ptr<BufferManager> Sptr;
    static Sptr make(const std::string &name)
    {
        Sptr m(new BufferManager());
        m->name = name;
        return m;
    }
    std::string name;
};

class Block {
public:
    Block() : yielded(false) {}
    virtual ~Block() { for (auto p : ins) delete p; }
    virtual void work() {}
    virtual void activate() {}
    virtual void propagateLabels(const InputPort *) {}
    void setupInput(size_t i) { while (ins.size() <= i) ins.push_back(new InputPort(int(ins.size()))); }
    void setupOutput(size_t) {}
    template <typename... A> void registerCall(A &&...) {}
    const std::vector<InputPort *> &inputs() const { return ins; }
    InputPort *input(size_t i) const { return ins.at(i); }
    OutputPort *output(size_t) { return &out; }
    std::string getName() const { return "WaveTrigger"; }
    void yield() { yielded = true; }
    // the driver's side
    std::vector<InputPort *> ins;
    OutputPort out;
    bool yielded;
};

struct BlockRegistry {
    template <typename F> BlockRegistry(const std::string &, F) {}
};

}  // namespace Pothos
