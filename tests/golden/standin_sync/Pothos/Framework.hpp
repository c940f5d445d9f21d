// Stand-in for <Pothos/Framework.hpp>: test infrastructure of this project, written new, not PothosCore.
//
// tests/golden/make_framesync_golden.py compiles a driver of its own against this header.  The driver includes digital/FrameSync.cpp of
// the reference BY PATH and runs its work() call after call.  The header holds exactly what that file uses, with bodies that RECORD: an
// input port hands out a typed pointer into the driver's stream and counts what is consumed, an output port hands out a typed pointer
// into the driver's output buffer and collects what is produced and posted.  The stand-in of the framers (tests/golden/standin) stays
// as it is; nothing here is shipped and nothing of the product includes it.
#pragma once
#include <complex>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <vector>

#define POTHOS_FCN_TUPLE(c, m) #m, &c::m

namespace Pothos {

struct Exception : std::runtime_error {
    Exception(const std::string &where, const std::string &what) : std::runtime_error(where + ": " + what) {}
};
struct InvalidArgumentException : Exception {
    InvalidArgumentException(const std::string &where, const std::string &what) : Exception(where, what) {}
};

struct DType {
    DType() : t(&typeid(void)) {}
    DType(const std::type_info &ti) : t(&ti) {}
    bool operator==(const DType &o) const { return *t == *o.t; }
    std::string toString() const { return t->name(); }
    const std::type_info *t;
};

//! what a label of the frame synchroniser carries: a floating value (the phase, kept as a double) or an unsigned integer (the length)
class Object {
public:
    Object() : is_double(false), real(0), number(0) {}
    Object(float v) : is_double(true), real(v), number(0) {}
    Object(double v) : is_double(true), real(v), number(0) {}
    Object(unsigned long v) : is_double(false), real(0), number(v) {}
    Object(unsigned long long v) : is_double(false), real(0), number(v) {}
    bool is_double;
    double real;
    unsigned long long number;
};

struct Label {
    std::string id;
    Object data;
    unsigned long long index;
    size_t width;
};

//! a port's memory as whatever pointer the block asks for
struct Buffer {
    void *p;
    template <typename T> operator T *() const { return static_cast<T *>(p); }
};

class InputPort {
public:
    InputPort() : mem(nullptr), count(0), consumed(0), reserve(0) {}
    Buffer buffer() const { return Buffer{const_cast<void *>(mem)}; }
    size_t elements() const { return count; }
    void consume(size_t n) { consumed += n; }
    void setReserve(size_t n) { reserve = n; }
    // the driver's side
    const void *mem;
    size_t count, consumed, reserve;
};

class OutputPort {
public:
    OutputPort() : mem(nullptr), count(0), produced(0) {}
    Buffer buffer() const { return Buffer{mem}; }
    size_t elements() const { return count; }
    void produce(size_t n) { produced += n; }
    void postLabel(const std::string &id, const Object &data, unsigned long long index, size_t width) { posted.push_back(Label{id, data, index, width}); }
    // the driver's side
    void *mem;
    size_t count, produced;
    std::vector<Label> posted;
};

struct WorkInfo {
    size_t minElements;
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
    virtual void activate() {}
    void setupInput(size_t, const DType &) {}
    void setupOutput(size_t, const DType &) {}
    template <typename... A> void registerCall(A &&...) {}
    InputPort *input(size_t) { return &in; }
    OutputPort *output(size_t) { return &out; }
    const WorkInfo &workInfo() const { return info; }
    // the driver's side: n_in elements at `src`, room for n_out at `dst`; the reserve stays as the block left it
    void give(const void *src, size_t n_in, void *dst, size_t n_out)
    {
        in.mem = src;
        in.count = n_in;
        in.consumed = 0;
        out.mem = dst;
        out.count = n_out;
        out.produced = 0;
        out.posted.clear();
        info.minElements = n_in < n_out ? n_in : n_out;
    }
    InputPort in;
    OutputPort out;
    WorkInfo info;
};

struct BlockRegistry {
    template <typename F> BlockRegistry(const std::string &, F) {}
};

}  // namespace Pothos
