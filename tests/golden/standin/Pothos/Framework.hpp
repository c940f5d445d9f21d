// Stand-in for <Pothos/Framework.hpp>: test infrastructure of this project, written new, not PothosCore.
//
// tests/golden/make_preamble_golden.py and make_framer_golden.py compile a driver of their own against this header.  The driver includes
// digital/PreambleCorrelator.cpp, digital/PreambleFramer.cpp and digital/FrameInsert.cpp of the reference BY PATH and runs their work().
// The header holds exactly what those three files use, with bodies that RECORD: an input port hands out one buffer and a list of labels,
// an output port collects the posted bytes and labels.  Nothing here is shipped and nothing of the product includes it.
//
// One check of its own: postBuffer() of a chunk that points into the input buffer requires the chunk to lie wholly inside it.  The
// reference's `label.index - consumed` wraps when a head would run backwards; such a chunk is never read: LeavesItsBuffer is thrown, the
// driver ends the case there and flags it.
#pragma once
#include <complex>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <utility>
#include <vector>

#define POTHOS_FCN_TUPLE(c, m) #m, &c::m

namespace Pothos {

struct Exception : std::runtime_error {
    Exception(const std::string &where, const std::string &what) : std::runtime_error(what), where(where) {}
    std::string where;
};
struct InvalidArgumentException : Exception {
    InvalidArgumentException(const std::string &where, const std::string &what) : Exception(where, what) {}
};

//! thrown by OutputPort::postBuffer: a chunk into the input that is not wholly inside it
struct LeavesItsBuffer {};

//! the element types of the three blocks
struct DType {
    DType() : t(&typeid(unsigned char)) {}
    DType(const std::type_info &ti) : t(&ti) {}
    size_t size() const
    {
        if (*t == typeid(unsigned char)) return 1;
        if (*t == typeid(std::complex<float>)) return sizeof(std::complex<float>);
        if (*t == typeid(std::complex<double>)) return sizeof(std::complex<double>);
        throw std::logic_error(std::string("stand-in DType: no size for ") + t->name());
    }
    bool operator==(const DType &o) const { return *t == *o.t; }
    std::string toString() const { return t->name(); }
    const std::type_info *t;
};

//! nothing, an unsigned integer or a string; only the integer converts to size_t
class Object {
public:
    enum Kind { NOTHING = 0, INTEGER = 1, STRING = 2 };
    Object() : kind(NOTHING), number(0) {}
    explicit Object(unsigned long long v) : kind(INTEGER), number(v) {}
    explicit Object(const std::string &s) : kind(STRING), number(0), text(s) {}
    bool canConvert(const std::type_info &ti) const { return kind == INTEGER and ti == typeid(size_t); }
    template <typename T> T convert() const
    {
        if (kind != INTEGER) throw std::logic_error("stand-in Object: convert() of something that is no integer");
        return T(number);
    }
    Kind kind;
    unsigned long long number;
    std::string text;
};

struct Label {
    Label() : index(0), width(1), ordinal(-1) {}
    Label(const std::string &id, const Object &data, unsigned long long index, size_t width = 1) : id(id), data(data), index(index), width(width), ordinal(-1) {}
    std::string id;
    Object data;
    unsigned long long index;
    size_t width;
    long ordinal;       // the stand-in's own: the place of the INPUT label this one was copied from, -1 for a label made by the block
};

//! memory by address and length in bytes; the (DType, n) constructor owns zero-initialised storage, copies share it
class BufferChunk {
public:
    BufferChunk() : address(0), length(0) {}
    BufferChunk(const DType &dtype, size_t numElems) : address(0), length(numElems * dtype.size()), dtype(dtype), store(new std::vector<unsigned char>(length ? length : 1, 0))
    {
        address = size_t(store->data());
    }
    size_t elements() const { return length / dtype.size(); }
    template <typename P> P as() const { return reinterpret_cast<P>(address); }
    template <typename T> operator T *() const { return reinterpret_cast<T *>(address); }
    size_t address;
    size_t length;
    DType dtype;
    std::shared_ptr<std::vector<unsigned char>> store;
};

class InputPort {
public:
    InputPort() : mem(0), count(0), consumed(0), reserve(0) {}
    BufferChunk takeBuffer() const
    {
        BufferChunk b;
        b.address = size_t(mem);
        b.length = count * dtype.size();
        b.dtype = dtype;
        return b;
    }
    const std::vector<Label> &labels() const { return held; }
    size_t elements() const { return count; }
    void consume(size_t n) { consumed += n; }
    void setReserve(size_t n) { reserve = n; }
    // the driver's side
    const unsigned char *mem;
    size_t count, consumed, reserve;
    DType dtype;
    std::vector<Label> held;
};

class OutputPort {
public:
    OutputPort() : in_lo(0), in_hi(0) {}
    const DType &dtype() const { return type; }
    void postBuffer(const BufferChunk &b)
    {
        if (b.length == 0) return;
        if (not b.store)        // a chunk that owns nothing came from takeBuffer(): into the input wholly, or not at all
        {
            if (b.address < in_lo or b.address > in_hi or b.length > in_hi - b.address) throw LeavesItsBuffer();
        }
        const unsigned char *p = reinterpret_cast<const unsigned char *>(b.address);
        bytes.insert(bytes.end(), p, p + b.length);
    }
    void postLabel(const Label &l) { posted.push_back(l); }
    void postLabel(const std::string &id, const Object &data, unsigned long long index) { posted.push_back(Label(id, data, index)); }
    // the driver's side
    DType type;
    size_t in_lo, in_hi;        // the input buffer's first byte and the byte behind its last
    std::vector<unsigned char> bytes;
    std::vector<Label> posted;
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
    virtual ~Block() {}
    virtual void work() {}
    void setupInput(size_t, const DType &d) { in.dtype = d; }
    void setupOutput(size_t, const DType &d, const std::string & = "") { out.type = d; }
    template <typename... A> void registerCall(A &&...) {}
    std::string uid() const { return "standin"; }
    InputPort *input(size_t) { return &in; }
    OutputPort *output(size_t) { return &out; }
    // the driver's side: one buffer of n elements and its labels in, a fresh record out
    void give(const void *mem, size_t n, const std::vector<Label> &labels)
    {
        in.mem = static_cast<const unsigned char *>(mem);
        in.count = n;
        in.consumed = 0;
        in.reserve = 0;
        in.held = labels;
        for (size_t i = 0; i < in.held.size(); i++) in.held[i].ordinal = long(i);
        out.in_lo = size_t(mem);
        out.in_hi = out.in_lo + n * in.dtype.size();
        out.bytes.clear();
        out.posted.clear();
    }
    InputPort in;
    OutputPort out;
};

struct BlockRegistry {
    template <typename F> BlockRegistry(const std::string &, F) {}
};

}  // namespace Pothos
