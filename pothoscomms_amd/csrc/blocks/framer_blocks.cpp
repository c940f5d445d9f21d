// framer_blocks.cpp -- the eleventh module of this port: the two framing blocks of the reference's digital/ directory,
// libpcx_framer_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source joins the
// DigitalBlocks module.
//
//   /comms/preamble_framer, /blocks/preamble_framer     digital/PreambleFramer.cpp:69-238
//   /comms/frame_insert, /blocks/frame_insert           digital/FrameInsert.cpp:82-340, digital/FrameHelper.hpp
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <complex>
#include <cstdint>
#include <cstring>
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

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_framer_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

// What the two blocks share: the handle, the two ids, the padding, the device and work().  Elem is the stream's element; a derived
// block keeps its own registerCall lines and one-line public calls (registerCall() cannot deduce a method of a base class).
template <typename Elem>
class FramerBase : public PortBlock {
protected:
    FramerBase(const std::string &who, const DType &dtype, int scalar, bool cplx, bool header, const std::string &endId)
        : PortBlock(who, kPortSlabBytes), _scalar(scalar), _cplx(cplx), _header(header), _preamble(1, Elem(1)), _symbolWidth(1), _headerId(0x55), _padding(0),
          _frameStartId("frameStart"), _frameEndId(endId), _h(nullptr)
    {
        check(pcx_framer_create(&_h, scalar, cplx ? 1 : 0), who + "()");
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
    }
    ~FramerBase() { pcx_framer_destroy(_h); }

    // every setting of the block on a handle
    int push(pcx_framer *h, const std::vector<Elem> &preamble, size_t width) const
    {
        int rc = pcx_framer_set_preamble(h, preamble.data(), preamble.size(), width, _header ? 1 : 0);
        if (rc == PCX_OK) rc = pcx_framer_set_header_id(h, _headerId);
        if (rc == PCX_OK) rc = pcx_framer_set_padding(h, _padding);
        return rc;
    }
    void preambleTo(const std::vector<Elem> &preamble, size_t width, const std::string &where)
    {
        check(pcx_framer_set_preamble(_h, preamble.data(), preamble.size(), width, _header ? 1 : 0), where);
        _preamble = preamble;
        _symbolWidth = width;
    }
    void headerIdTo(unsigned char id)
    {
        check(pcx_framer_set_header_id(_h, id), _who + "::setHeaderId()");
        _headerId = id;
    }
    void paddingTo(size_t size)
    {
        check(pcx_framer_set_padding(_h, size), _who + "::setPaddingSize()");
        _padding = size;
    }
    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with the settings
    void deviceTo(const size_t device)
    {
        const std::string where = _who + "::setDevice()";
        const int d = checkedDevice(device);
        OnDevice on(d, where.c_str());
        pcx_framer *fresh = nullptr;
        check(pcx_framer_create(&fresh, _scalar, _cplx ? 1 : 0), where);
        const int rc = push(fresh, _preamble, _symbolWidth);
        if (rc != PCX_OK) { pcx_framer_destroy(fresh); check(rc, where); }
        pcx_framer_destroy(_h);
        _h = fresh;
        _device = d;
    }

public:
    // work (PreambleFramer.cpp:138-216, FrameInsert.cpp:183-288).  The reference forwards slices of its input buffer and posts its
    // preamble and padding buffers between them; here the labels become events, the host plans the call against the room of the output
    // port's buffer and one kernel writes the framed stream there.  Labels the plan did not handle stay with the
    // input they sit on, for the next call.
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t in = inPort->elements(), cap = outPort->elements();
        if (in == 0 || cap == 0) return;
        _events.clear();
        for (const auto &label : inPort->labels()) {
            pcx_frame_event e;
            e.index = label.index;
            e.width = label.width;
            e.kind = label.id == _frameStartId ? PCX_FRAME_START : label.id == _frameEndId ? PCX_FRAME_END : PCX_FRAME_OTHER;   // the start id first
            e.length = 0;
            if (_header && e.kind == PCX_FRAME_START && label.data.canConvert(typeid(size_t)))     // FrameInsert.cpp:231-234
                e.length = (uint32_t)((label.data.template convert<size_t>() * label.width) & 0xffffu);
            _events.push_back(e);
        }
        const size_t n = _events.size();
        _used.assign(n, 0);
        _at.assign(n, 0);
        _shift.assign(n, 0);
        pcx_frame_plan plan;
        check(pcx_framer_process(_h, inPort->buffer().template as<const void *>(), in, _events.data(), n, outPort->buffer().template as<void *>(), cap, &plan,
                                 _used.data(), _at.data(), _shift.data()),
              _who + "::work()");
        size_t k = 0;
        for (const auto &label : inPort->labels()) {
            if (_used[k]) {
                pcxfw::Label shifted(label);
                shifted.index += _shift[k];
                outPort->postLabel(shifted);
            }
            k++;
        }
        inPort->consume((size_t)plan.consumed);
        outPort->produce((size_t)plan.out_len);
    }
    // the labels are posted by work() (PreambleFramer.cpp:218-221, FrameInsert.cpp:290-293)
    void propagateLabels(const pcxfw::InputPort *) {}

protected:
    const int _scalar;
    const bool _cplx, _header;
    std::vector<Elem> _preamble;
    size_t _symbolWidth;
    unsigned char _headerId;
    size_t _padding;
    std::string _frameStartId, _frameEndId;
    pcx_framer *_h;
    std::vector<pcx_frame_event> _events;
    std::vector<unsigned char> _used;
    std::vector<uint64_t> _at, _shift;
};

/***********************************************************************
 * |PothosDoc Preamble Framer
 *
 * Puts a known symbol pattern in front of every frame: wherever a label with the frame start ID sits on the byte stream arriving on
 * input 0, the GPU writes the preamble ahead of the labelled symbol, and everything else passes through to output 0 in order.  The
 * preamble correlator of a receiver looks for this pattern.
 *
 * With a frame end ID set, zero symbols are appended behind the symbol that carries the end label, as many as the padding size says.
 *
 * <h2>Where the labels go</h2>
 *
 * A start label, and any label sharing its index, ends up on the first symbol of the inserted preamble.  An end label, and any label
 * sharing its index, ends up on the last symbol of the padding.  Every other label keeps pointing at the symbol it pointed at.
 *
 * <h2>Symbols of any width</h2>
 *
 * A symbol is one byte whatever number of bits it carries, so a stream of single bits is framed the same way with a preamble of
 * zeros and ones.
 *
 * |category /Digital
 * |keywords bit symbol preamble frame
 * |alias /blocks/preamble_framer
 *
 * |param preamble The symbol pattern to insert, one entry per symbol, each as wide as the symbols of the stream.
 * |default [1]
 *
 * |param frameStartId[Frame Start ID] Name of the label that sits on the first symbol of a frame's data.
 * |default "frameStart"
 * |widget StringEntry()
 *
 * |param frameEndId[Frame End ID] Name of the label that sits on the last symbol of a frame's data.
 * Padding is appended only behind such a label; leave the name empty and nothing is appended.
 * |default ""
 * |widget StringEntry()
 * |preview valid
 *
 * |param paddingSize[Padding Size] How many zero symbols follow a frame whose end label was found.
 * |default 0
 * |preview valid
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * Larger slabs carry more symbols per call (throughput), smaller ones return sooner (latency).
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/preamble_framer()
 * |setter setPreamble(preamble)
 * |setter setFrameStartId(frameStartId)
 * |setter setFrameEndId(frameEndId)
 * |setter setPaddingSize(paddingSize)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class PreambleFramer : public FramerBase<unsigned char> {
public:
    PreambleFramer() : FramerBase<unsigned char>("PreambleFramer", DType(typeid(unsigned char)), PCX_U8, false, false, "")      // PreambleFramer.cpp:89-91
    {
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, setPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, getPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, setFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, getFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, setFrameEndId));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, getFrameEndId));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, setPaddingSize));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, getPaddingSize));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(PreambleFramer, getPortSlabBytes));
    }
    void setPreamble(const std::vector<unsigned char> preamble)
    {
        if (preamble.empty()) throw InvalidArgumentException("PreambleFramer::setPreamble()", "preamble cannot be empty");
        preambleTo(preamble, 1, "PreambleFramer::setPreamble()");
    }
    std::vector<unsigned char> getPreamble() const { return _preamble; }
    void setFrameStartId(std::string id) { _frameStartId = id; }
    std::string getFrameStartId() const { return _frameStartId; }
    void setFrameEndId(std::string id) { _frameEndId = id; }
    std::string getFrameEndId() const { return _frameEndId; }
    void setPaddingSize(const size_t size) { paddingTo(size); }
    size_t getPaddingSize() const { return _padding; }
    void setDevice(const size_t device) { deviceTo(device); }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }
};

/***********************************************************************
 * |PothosDoc Frame Insert
 *
 * Opens every frame of a stream of complex samples with a synchronization header: wherever a label with the frame start ID sits on
 * the stream arriving on input 0, the GPU writes the preamble, each of its symbols held for the symbol width, and behind it 58 BPSK
 * symbols that spell the header ID, the frame length and a checksum, each nibble protected by a Hamming code.  A Frame Sync block
 * at the receiver finds frames by this header and corrects frequency and phase with it.  A frame end label appends zero samples.
 *
 * The frame length comes from the start label: its data times its width, when the data is a number.
 *
 * <h2>Where the labels go</h2>
 *
 * A start label, and any label sharing its index, ends up on the first sample of the inserted header.  An end label, and any label
 * sharing its index, ends up on the last sample of the padding.  Every other label keeps pointing at the sample it pointed at.
 *
 * |category /Digital
 * |keywords preamble frame sync
 * |alias /blocks/frame_insert
 *
 * |param dtype[Data Type] Element type of the stream, the same on the input and on the output.
 * |widget DTypeChooser(cfloat=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param preamble The symbols of the synchronization word, in the order they are sent.
 * |default [1, 1, -1]
 * |option [Barker Code 2] \[1, -1\]
 * |option [Barker Code 3] \[1, 1, -1\]
 * |option [Barker Code 4] \[1, 1, -1, 1\]
 * |option [Barker Code 5] \[1, 1, 1, -1, 1\]
 *
 * |param headerId [Header ID] An 8-bit number written into every header.
 * A receiver drops the frames whose number it does not expect.
 * |default 0x55
 *
 * |param symbolWidth [Symbol Width] For how many samples each preamble symbol is held.
 * This has nothing to do with the samples per symbol of the payload's modulation; a synchronization word is usually much slower.
 * |default 20
 * |units samples
 *
 * |param frameStartId[Frame Start ID] Name of the label that sits on the first sample of a frame's data.
 * |default "frameStart"
 * |widget StringEntry()
 *
 * |param frameEndId[Frame End ID] Name of the label that sits on the last sample of a frame's data.
 * |default "frameEnd"
 * |widget StringEntry()
 *
 * |param paddingSize[Padding Size] How many zero samples follow a frame whose end label was found; 0 appends nothing.
 * |default 0
 * |preview valid
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
 * |factory /comms/frame_insert(dtype)
 * |setter setPreamble(preamble)
 * |setter setHeaderId(headerId)
 * |setter setSymbolWidth(symbolWidth)
 * |setter setFrameStartId(frameStartId)
 * |setter setFrameEndId(frameEndId)
 * |setter setPaddingSize(paddingSize)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class FrameInsert : public FramerBase<std::complex<T>> {
    typedef FramerBase<std::complex<T>> Base;

public:
    FrameInsert(const DType &dtype, int scalar) : Base("FrameInsert", dtype, scalar, true, true, "frameEnd")      // FrameInsert.cpp:111-115
    {
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setHeaderId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getHeaderId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setSymbolWidth));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getSymbolWidth));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setFrameEndId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getFrameEndId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setPaddingSize));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getPaddingSize));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(FrameInsert, getPortSlabBytes));
        this->preambleTo(this->_preamble, 20, "FrameInsert()");      // preamble {1}, each symbol 20 samples wide
    }
    // (the symbols arrive as complex doubles and are rounded to the stream's type, as a Pothos call converts them)
    void setPreamble(const std::vector<std::complex<double>> preamble)
    {
        if (preamble.empty()) throw InvalidArgumentException("FrameInsert::setPreamble()", "preamble cannot be empty");
        std::vector<std::complex<T>> typed;
        for (const auto &s : preamble) typed.push_back(std::complex<T>((T)s.real(), (T)s.imag()));
        this->preambleTo(typed, this->_symbolWidth, "FrameInsert::setPreamble()");
    }
    std::vector<std::complex<double>> getPreamble() const
    {
        std::vector<std::complex<double>> out;
        for (const auto &s : this->_preamble) out.push_back(std::complex<double>(s.real(), s.imag()));
        return out;
    }
    void setHeaderId(const unsigned char id) { this->headerIdTo(id); }
    unsigned char getHeaderId() const { return this->_headerId; }
    void setSymbolWidth(const size_t width)
    {
        if (width == 0) throw InvalidArgumentException("FrameInsert::setSymbolWidth()", "symbol width cannot be 0");
        this->preambleTo(this->_preamble, width, "FrameInsert::setSymbolWidth()");
    }
    size_t getSymbolWidth() const { return this->_symbolWidth; }
    void setFrameStartId(std::string id) { this->_frameStartId = id; }
    std::string getFrameStartId() const { return this->_frameStartId; }
    void setFrameEndId(std::string id) { this->_frameEndId = id; }
    std::string getFrameEndId() const { return this->_frameEndId; }
    void setPaddingSize(const size_t size) { this->paddingTo(size); }
    size_t getPaddingSize() const { return this->_padding; }
    void setDevice(const size_t device) { this->deviceTo(device); }
    size_t getDevice() const { return this->_device < 0 ? 0 : (size_t)this->_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { this->checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return this->_slabBytes; }
};

Block *PreambleFramerFactory() { return new PreambleFramer(); }
pcxfw::BlockRegistry registerPreambleFramer("/comms/preamble_framer", &PreambleFramerFactory);
pcxfw::BlockRegistry registerPreambleFramerOldPath("/blocks/preamble_framer", &PreambleFramerFactory);

// FrameInsertFactory (FrameInsert.cpp:326-334): the two complex floating types
Block *FrameInsertFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && cplx && dtype.dimension() == 1) {
        if (scalar == PCX_F64) return new FrameInsert<double>(dtype, scalar);
        if (scalar == PCX_F32) return new FrameInsert<float>(dtype, scalar);
    }
    throw InvalidArgumentException("FrameInsertFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerFrameInsert("/comms/frame_insert", &FrameInsertFactory);
pcxfw::BlockRegistry registerFrameInsertOldPath("/blocks/frame_insert", &FrameInsertFactory);

}  // namespace
