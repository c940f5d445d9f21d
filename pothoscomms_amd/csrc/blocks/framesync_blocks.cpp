// framesync_blocks.cpp -- the sixteenth module of this port: the frame synchroniser of the reference's digital/ directory,
// libpcx_framesync_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source joins the
// DigitalBlocks module.
//
//   /comms/frame_sync, /blocks/frame_sync     digital/FrameSync.cpp:143-762, digital/FrameHelper.hpp
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
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

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes)
constexpr size_t kPortSlabBytes = 64u << 20;

const char *const kModes[] = {"RAW", "PHASE", "TIMING", "DEBUG"};

/***********************************************************************
 * |PothosDoc Frame Sync
 *
 * The receiving end of the Frame Insert block.  The GPU slides over the complex samples arriving on input 0 and, at every sample
 * offset, asks whether a synchronization word begins there: is the envelope steady, what carrier offset do the samples of the last
 * preamble symbol show, and how well does the whole word correlate once that offset is taken out.  Where the correlation peaks and no
 * larger peak follows for half a word, the 58 header symbols behind the word are read, their Hamming code is checked, and a header
 * with the expected ID and a length opens a frame.  Its payload goes to output 0; everything outside of frames is dropped.
 *
 * <h2>What is done to the payload</h2>
 *
 * <b>RAW</b> only scales the samples to unit amplitude, for a receiver that tracks carrier and timing itself; the phase offset label
 * tells its loop where to start.  <b>PHASE</b> also turns every sample back by the carrier phase that the header search estimated,
 * advancing with the estimated frequency offset.  <b>TIMING</b> does the same and keeps one sample per data symbol, taken where the
 * first header symbol was strongest.  <b>DEBUG</b> is PHASE from the first sample of the synchronization word on, to look at.
 * The estimates are made once per frame; long payloads or drifting oscillators want tracking blocks behind this one.
 *
 * <h2>Labels</h2>
 *
 * Up to three labels mark a frame on the output: the phase offset (a double, radians) and the frame start (the payload length in
 * symbols) on the first payload element, the frame end (the length again) on the last.  A label whose ID is empty is not posted.
 * Their width is the data width, or 1 in TIMING mode.  Labels of the input are dropped.
 *
 * |category /Digital
 * |keywords preamble frame sync timing offset recover
 * |alias /blocks/frame_sync
 *
 * |param dtype[Data Type] Element type of the stream, the same on the input and on the output.
 * |widget DTypeChooser(cfloat=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param outputMode[Output Mode] What is done to the payload samples on their way out.
 * |default "RAW"
 * |option [Raw symbols] "RAW"
 * |option [Phase correction] "PHASE"
 * |option [Timing recovery] "TIMING"
 * |option [Debug preamble] "DEBUG"
 *
 * |param preamble The symbols of the synchronization word, as the frame inserter sends them.
 * |default [1, 1, -1]
 * |option [Barker Code 2] \[1, -1\]
 * |option [Barker Code 3] \[1, 1, -1\]
 * |option [Barker Code 4] \[1, 1, -1, 1\]
 * |option [Barker Code 5] \[1, 1, 1, -1, 1\]
 *
 * |param headerId [Header ID] The 8-bit number a header must carry; frames with another number are passed over.
 * |default 0x55
 *
 * |param symbolWidth [Symbol Width] For how many data symbols each preamble symbol is held: the frame inserter's symbol width.
 * At least 3.
 * |default 20
 * |units samples
 *
 * |param dataWidth [Data Width] Samples per data symbol on this block's input.
 * |default 4
 * |units samples
 *
 * |param inputThreshold [Input Threshold] Amplitude below which the input counts as noise and is not searched.
 * |default 0.01
 *
 * |param frameStartId[Frame Start ID] Name of the label on the first element of a frame's payload; it carries the payload length.
 * |default "frameStart"
 * |widget StringEntry()
 * |preview valid
 * |tab Labels
 *
 * |param frameEndId[Frame End ID] Name of the label on the last element of a frame's payload; empty: no such label.
 * |default ""
 * |widget StringEntry()
 * |preview valid
 * |tab Labels
 *
 * |param phaseOffsetID[Phase Offset ID] Name of the label that carries the carrier phase at the first payload element; empty: no such label.
 * |default ""
 * |widget StringEntry()
 * |preview valid
 * |tab Labels
 *
 * |param verboseMode[Verbose Mode] Accepted for compatibility; this block prints nothing.
 * |default false
 * |preview disable
 * |option [Enable] true
 * |option [Disable] false
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
 * |factory /comms/frame_sync(dtype)
 * |setter setOutputMode(outputMode)
 * |setter setPreamble(preamble)
 * |setter setHeaderId(headerId)
 * |setter setSymbolWidth(symbolWidth)
 * |setter setDataWidth(dataWidth)
 * |setter setFrameStartId(frameStartId)
 * |setter setFrameEndId(frameEndId)
 * |setter setPhaseOffsetID(phaseOffsetID)
 * |setter setInputThreshold(inputThreshold)
 * |setter setVerboseMode(verboseMode)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
template <typename T>
class FrameSync : public PortBlock {
public:
    FrameSync(const DType &dtype, int scalar)
        : PortBlock("FrameSync", kPortSlabBytes), _scalar(scalar), _mode("RAW"), _preamble(1, std::complex<T>(1)), _headerId(0x55), _symbolWidth(20), _dataWidth(4),
          _threshold((T)0.01), _verbose(false), _frameStartId("frameStart"), _h(nullptr)
    {
        check(pcx_fsync_create(&_h, scalar, 1), "FrameSync()");
        Block::setupInput(0, dtype, kDomain);
        Block::setupOutput(0, dtype, kDomain);
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setOutputMode));      // FrameSync.cpp:165-183
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getOutputMode));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getPreamble));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setHeaderId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getHeaderId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setSymbolWidth));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getSymbolWidth));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setDataWidth));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getDataWidth));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getFrameStartId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setFrameEndId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getFrameEndId));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setPhaseOffsetID));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getPhaseOffsetID));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setInputThreshold));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getInputThreshold));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setVerboseMode));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(FrameSync, getPortSlabBytes));
    }
    ~FrameSync() { pcx_fsync_destroy(_h); }

    void setOutputMode(const std::string &mode)
    {
        check(pcx_fsync_set_output_mode(_h, modeCode(mode)), "FrameSync::setOutputMode(" + mode + ")");
        _mode = mode;
    }
    std::string getOutputMode() const { return _mode; }
    // (the symbols arrive as complex doubles and are rounded to the stream's type, as a Pothos call converts them)
    void setPreamble(const std::vector<std::complex<double>> preamble)
    {
        if (preamble.empty()) throw InvalidArgumentException("FrameSync::setPreamble()", "preamble cannot be empty");
        std::vector<std::complex<T>> typed;
        for (const auto &s : preamble) typed.push_back(std::complex<T>((T)s.real(), (T)s.imag()));
        check(pcx_fsync_set_preamble(_h, typed.data(), typed.size()), "FrameSync::setPreamble()");
        _preamble = typed;
    }
    std::vector<std::complex<double>> getPreamble() const
    {
        std::vector<std::complex<double>> out;
        for (const auto &s : _preamble) out.push_back(std::complex<double>(s.real(), s.imag()));
        return out;
    }
    void setHeaderId(const unsigned char id)
    {
        check(pcx_fsync_set_header_id(_h, id), "FrameSync::setHeaderId()");
        _headerId = id;
    }
    unsigned char getHeaderId() const { return _headerId; }
    void setSymbolWidth(const size_t width)
    {
        if (width == 0) throw InvalidArgumentException("FrameSync::setSymbolWidth()", "symbol width cannot be 0");
        check(pcx_fsync_set_symbol_width(_h, width), "FrameSync::setSymbolWidth()");
        _symbolWidth = width;
    }
    size_t getSymbolWidth() const { return _symbolWidth; }
    void setDataWidth(const size_t width)
    {
        if (width < 2) throw InvalidArgumentException("FrameSync::setDataWidth()", "data width should be at least 2 samples per symbol");
        check(pcx_fsync_set_data_width(_h, width), "FrameSync::setDataWidth()");
        _dataWidth = width;
    }
    size_t getDataWidth() const { return _dataWidth; }
    void setFrameStartId(std::string id) { idTo(PCX_FSYNC_FRAME_START, id, _frameStartId); }
    std::string getFrameStartId() const { return _frameStartId; }
    void setFrameEndId(std::string id) { idTo(PCX_FSYNC_FRAME_END, id, _frameEndId); }
    std::string getFrameEndId() const { return _frameEndId; }
    void setPhaseOffsetID(std::string id) { idTo(PCX_FSYNC_PHASE_OFFSET, id, _phaseOffsetId); }
    std::string getPhaseOffsetID() const { return _phaseOffsetId; }
    // (a double on the wire, kept in the stream's precision as the reference's RealType argument is)
    void setInputThreshold(const double threshold)
    {
        if ((T)threshold < 0) throw InvalidArgumentException("FrameSync::setInputThreshold()", "threshold should be non-negative");
        check(pcx_fsync_set_input_threshold(_h, threshold), "FrameSync::setInputThreshold()");
        _threshold = (T)threshold;
    }
    double getInputThreshold() const { return _threshold; }
    void setVerboseMode(const bool enb)
    {
        check(pcx_fsync_set_verbose(_h, enb ? 1 : 0), "FrameSync::setVerboseMode()");
        _verbose = enb;
    }
    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with the settings
    void setDevice(const size_t device)
    {
        const std::string where = "FrameSync::setDevice()";
        const int d = checkedDevice(device);
        OnDevice on(d, where.c_str());
        pcx_fsync *fresh = nullptr;
        check(pcx_fsync_create(&fresh, _scalar, 1), where);
        const int rc = push(fresh);
        if (rc != PCX_OK) { pcx_fsync_destroy(fresh); check(rc, where); }
        pcx_fsync_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    // always a circular buffer on the input (FrameSync.cpp:320-324): the search slides a window over the stream
    pcxfw::BufferManager::Sptr getInputBufferManager(const std::string &, const std::string &domain)
    {
#ifdef PCX_WITH_POTHOS
        (void)domain;
        return Pothos::BufferManager::make("circular");
#else
        const std::string where = "FrameSync::getInputBufferManager()";
        OnDevice on(_device, where.c_str());
        return manager(domain == kDomain, "circular");
#endif
    }

    void activate() { check(pcx_fsync_activate(_h), "FrameSync::activate()"); }

    // work (FrameSync.cpp:390-590): one call of the handle; what it consumed, produced, asks to be reserved and posts comes back in the
    // result.  Labels of the input are dropped (:309-318).
    void work()
    {
        auto inPort = this->input(0);
        auto outPort = this->output(0);
        const size_t in = inPort->elements(), cap = outPort->elements();
        pcx_fsync_result r;
        check(pcx_fsync_process(_h, in ? inPort->buffer().template as<const void *>() : nullptr, in, cap ? outPort->buffer().template as<void *>() : nullptr, cap, &r),
              "FrameSync::work()");
        for (uint32_t k = 0; k < r.n_labels; k++) {
            const pcx_fsync_label &l = r.labels[k];
            if (l.kind == PCX_FSYNC_PHASE_OFFSET) outPort->postLabel(pcxfw::Label(_phaseOffsetId, pcxfw::Object(l.value), (size_t)l.index, (size_t)l.width));
            else
                outPort->postLabel(pcxfw::Label(l.kind == PCX_FSYNC_FRAME_START ? _frameStartId : _frameEndId, pcxfw::Object((size_t)l.length), (size_t)l.index,
                                                (size_t)l.width));
        }
        inPort->setReserve((size_t)r.reserve);
        inPort->consume((size_t)r.consumed);
        outPort->produce((size_t)r.produced);
    }
    void propagateLabels(const pcxfw::InputPort *) {}

private:
    static int modeCode(const std::string &mode)
    {
        for (int k = 0; k < 4; k++)
            if (mode == kModes[k]) return k;
        throw InvalidArgumentException("FrameSync::setOutputMode(" + mode + ")", "unknown output mode");
    }
    void idTo(int kind, const std::string &id, std::string &mine)
    {
        check(pcx_fsync_set_label_id(_h, kind, id.c_str()), "FrameSync::setLabelId()");
        mine = id;
    }
    // every setting of the block on a handle
    int push(pcx_fsync *h) const
    {
        int rc = pcx_fsync_set_output_mode(h, modeCode(_mode));
        if (rc == PCX_OK) rc = pcx_fsync_set_symbol_width(h, _symbolWidth);
        if (rc == PCX_OK) rc = pcx_fsync_set_data_width(h, _dataWidth);
        if (rc == PCX_OK) rc = pcx_fsync_set_preamble(h, _preamble.data(), _preamble.size());
        if (rc == PCX_OK) rc = pcx_fsync_set_header_id(h, _headerId);
        if (rc == PCX_OK) rc = pcx_fsync_set_input_threshold(h, _threshold);
        if (rc == PCX_OK) rc = pcx_fsync_set_verbose(h, _verbose ? 1 : 0);
        if (rc == PCX_OK) rc = pcx_fsync_set_label_id(h, PCX_FSYNC_FRAME_START, _frameStartId.c_str());
        if (rc == PCX_OK) rc = pcx_fsync_set_label_id(h, PCX_FSYNC_FRAME_END, _frameEndId.c_str());
        if (rc == PCX_OK) rc = pcx_fsync_set_label_id(h, PCX_FSYNC_PHASE_OFFSET, _phaseOffsetId.c_str());
        return rc;
    }

    const int _scalar;
    std::string _mode;
    std::vector<std::complex<T>> _preamble;
    unsigned char _headerId;
    size_t _symbolWidth, _dataWidth;
    T _threshold;
    bool _verbose;
    std::string _frameStartId, _frameEndId, _phaseOffsetId;
    pcx_fsync *_h;
};

// FrameSyncFactory (FrameSync.cpp:748-756): the two complex floating types
Block *FrameSyncFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && cplx && dtype.dimension() == 1) {
        if (scalar == PCX_F64) return new FrameSync<double>(dtype, scalar);
        if (scalar == PCX_F32) return new FrameSync<float>(dtype, scalar);
    }
    throw InvalidArgumentException("FrameSyncFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerFrameSync("/comms/frame_sync", &FrameSyncFactory);
pcxfw::BlockRegistry registerFrameSyncOldPath("/blocks/frame_sync", &FrameSyncFactory);

}  // namespace
