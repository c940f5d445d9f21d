// trigger_blocks.cpp -- the seventeenth module of this port: libpcx_trigger_blocks.so (with the runner ABI of include/pcx_blocks.h
// linked in).  In a PothosComms build this source joins the UtilityBlocks module.
//
//   /comms/wave_trigger, /blocks/wave_trigger     utility/WaveTrigger.cpp:163-777
//
// Built against pcx_framework.hpp: PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "pcx.h"
#include "pcx_block_util.hpp"
#include "pcx_framework.hpp"

using pcxfw::Block;
using pcxfw::BufferChunk;
using pcxfw::DType;
using pcxfw::InvalidArgumentException;
using pcxfw::Label;
using pcxfw::Object;
using pcxfw::Packet;

namespace {

using namespace pcxblk;     // check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes)
constexpr size_t kPortSlabBytes = 64u << 20;

// DType element name -> (pcx_scalar, complex?): the sixteen types the search converts to float
bool parseTriggerType(const DType &dt, int &scalar, bool &cplx)
{
    if (parseElemType(dt, scalar, cplx)) return true;
    const std::string n = dt.name();
    cplx = false;
    if (n == "uint64") scalar = PCX_U64;
    else if (n == "uint32") scalar = PCX_U32;
    else if (n == "uint16") scalar = PCX_U16;
    else if (n == "uint8") scalar = PCX_U8;
    else return false;
    return true;
}

void releasePinned(void *p) { (void)pcx_host_free(p); }
// `elems` elements of page-locked host memory: what a captured window is written into (and what a packet then carries away)
BufferChunk pinnedChunk(const DType &dt, size_t elems)
{
#ifdef PCX_WITH_POTHOS
    return BufferChunk(dt, elems);
#else
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(elems * dt.size(), 1);
    check(pcx_host_alloc(&p, bytes), "WaveTrigger::work()");
    return BufferChunk::adopt(p, elems * dt.size(), dt, &releasePinned);
#endif
}

/***********************************************************************
 * |PothosDoc Wave Trigger
 *
 * Watches one of its input ports for a trigger: a crossing of a level with a chosen slope, a label, or a timer.
 * On a trigger the block cuts the same stretch of samples out of every input port and posts it on output 0 as one Packet
 * per port; the streams themselves are consumed and go nowhere else.  The level search and the cut run on the GPU on the
 * buffers where they lie, so of a chain that lives in device memory only the posted samples reach the host.
 * Messages that arrive on an input are passed on to the output.
 *
 * <h2>The packets</h2>
 * The payload holds <em>numPoints</em> samples of the port's type, beginning <em>position</em> samples in front of the trigger.
 * The metadata holds "index" (the input port), "position" (where in the payload the trigger lies, with its fraction)
 * and "level".  The labels of the cut stretch come along, and a label "T" marks the trigger when a level crossing made it.
 *
 * <h2>Windows</h2>
 * With <em>numWindows</em> above 1 a packet is put together from that many triggers in a row, numPoints / numWindows samples each;
 * the search for the next one begins behind the window, the hold-off and the position.
 *
 * |category /Utility
 * |alias /blocks/wave_trigger
 *
 * |param numPorts[Num Ports] How many input ports the block has.
 * |default 1
 * |widget SpinBox(minimum=1)
 * |preview disable
 *
 * |param numPoints[Num Points] Samples per packet.
 * |default 1024
 * |widget SpinBox(minimum=0)
 *
 * |param numWindows[Windows] Triggers per packet, back to back.
 * |default 1
 * |widget SpinBox(minimum=1)
 *
 * |param eventRate[Event Rate] The most packets per second; samples in between are dropped.
 * In automatic mode a trigger is forced when none came for one and a half periods of this rate.
 * |units events/sec
 * |default 1.0
 *
 * |param alignment[Alignment] Whether all ports are consumed in step, or the ports other than the source run free.
 * |default false
 * |option [Disable] false
 * |option [Enable] true
 *
 * |param source[Source] The input port that is searched.
 * |default 0
 * |widget SpinBox(minimum=0)
 *
 * |param holdOff[Hold Off] Samples after a window during which nothing triggers.
 * |units samples
 * |default 0
 * |preview valid
 *
 * |param slope[Slope] Rising through the level (POS), falling through it (NEG), or either (LEVEL).
 * |default "POS"
 * |option [Positive] "POS"
 * |option [Negative] "NEG"
 * |option [Level] "LEVEL"
 *
 * |param mode [Mode] AUTOMATIC: search, and force a trigger by timer when none comes.
 * SEMIAUTOMATIC: the same, but the timer only acts on the windows after the first.
 * NORMAL: search only.  PERIODIC: no search, the timer alone.  DISABLED: nothing is posted.
 * |default "AUTOMATIC"
 * |option [Automatic] "AUTOMATIC"
 * |option [Semi-automatic] "SEMIAUTOMATIC"
 * |option [Normal] "NORMAL"
 * |option [Periodic] "PERIODIC"
 * |option [Disabled] "DISABLED"
 *
 * |param level [Level] The value the source has to cross.
 * |default 0.0
 * |widget DoubleSpinBox()
 *
 * |param position [Position] Samples of the packet in front of the trigger.
 * |units samples
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview valid
 *
 * |param labelId [Label ID] When not empty, a label of this id on the source port triggers instead of the level.
 * |default ""
 * |widget StringEntry()
 * |preview valid
 *
 * |param device[Device] Ordinal of the GPU that carries the block.
 * |default 0
 * |widget SpinBox(minimum=0)
 * |preview disable
 * |tab Device
 *
 * |param portSlabBytes[Port Slab Bytes] Size of the page-locked port buffers the block asks the framework for.
 * |default 67108864
 * |units bytes
 * |preview disable
 * |tab Device
 *
 * |factory /comms/wave_trigger()
 * |initializer setNumPorts(numPorts)
 * |setter setNumPoints(numPoints)
 * |setter setNumWindows(numWindows)
 * |setter setEventRate(eventRate)
 * |setter setAlignment(alignment)
 * |setter setSource(source)
 * |setter setHoldOff(holdOff)
 * |setter setSlope(slope)
 * |setter setMode(mode)
 * |setter setLevel(level)
 * |setter setPosition(position)
 * |setter setLabelId(labelId)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class WaveTrigger : public PortBlock {
public:
    typedef std::chrono::high_resolution_clock Clock;

    static Block *make() { return new WaveTrigger(); }

    WaveTrigger()
        : PortBlock("WaveTrigger", kPortSlabBytes), _numPoints(0), _numWindows(1), _eventRate(1.0), _alignment(true), _source(0), _holdOff(0),
          _slopeCode(PCX_TRIGGER_POS), _timerOn(false), _windowTimerOn(false), _periodic(false), _searchOn(false), _level(0.0), _position(0),
          _fromLevel(false), _pointsRemaining(0), _windowsRemaining(0), _holdOffRemaining(0), _eventOffset(0.0)
    {
        Block::setupInput(0, DType(), kDomain);
        Block::setupOutput(0);
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setNumPorts));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setNumPoints));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getNumPoints));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setNumWindows));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getNumWindows));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setEventRate));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getEventRate));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setAlignment));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getAlignment));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setHoldOff));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getHoldOff));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setSource));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getSource));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setSlope));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getSlope));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setMode));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getMode));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setLevel));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getLevel));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setPosition));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getPosition));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setLabelId));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getLabelId));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setIdsList));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(WaveTrigger, getPortSlabBytes));

        // the reference's constructor values (WaveTrigger.cpp:216-225)
        this->setNumPoints(1024);
        this->setNumWindows(1);
        this->setEventRate(1.0);
        this->setAlignment(true);
        this->setSource(0);
        this->setHoldOff(1024);
        this->setSlope("POS");
        this->setMode("AUTOMATIC");
        this->setLevel(0.5);
        this->setPosition(128);
    }
    ~WaveTrigger() { dropHandles(); }

    void setNumPorts(const size_t numPorts)
    {
        for (size_t i = this->inputs().size(); i < numPorts; i++) Block::setupInput(i, DType(), kDomain);
    }

    void setNumPoints(const size_t numPoints)
    {
        if (numPoints == 0) throw InvalidArgumentException("WaveTrigger::setNumPoints()", "num points must be positive");
        _numPoints = numPoints;
    }
    size_t getNumPoints() const { return _numPoints; }

    // DIFFERENCE: 0 is refused with the words the reference meant to use; it tests the OLD value (WaveTrigger.cpp:246) and work()
    // then divides by zero (:522)
    void setNumWindows(const size_t numWindows)
    {
        if (numWindows == 0) throw InvalidArgumentException("WaveTrigger::setNumWindows()", "num windows must be positive");
        _numWindows = numWindows;
    }
    size_t getNumWindows() const { return _numWindows; }

    void setAlignment(const bool enabled) { _alignment = enabled; }
    bool getAlignment() const { return _alignment; }

    // a hold-off that is running is cut down to the new value (WaveTrigger.cpp:270)
    void setHoldOff(const size_t holdOff)
    {
        _holdOff = holdOff;
        _holdOffRemaining = std::min(_holdOffRemaining, _holdOff);
    }
    // (bool as in the reference, WaveTrigger.cpp:273, :284: "is there a hold-off", "is the source another port than 0")
    bool getHoldOff() const { return _holdOff; }

    void setSource(const size_t channel)
    {
        if (channel >= this->inputs().size()) throw InvalidArgumentException("WaveTrigger::setSource()", "channel out of range");
        _source = channel;
    }
    bool getSource() const { return _source; }

    void setEventRate(const double rate)
    {
        if (rate <= 0.0) throw InvalidArgumentException("WaveTrigger::setEventRate()", "event rate must be positive");
        _eventRate = rate;
        _eventOff = std::chrono::duration_cast<Clock::duration>(std::chrono::nanoseconds((long long)(1e9 / _eventRate)));
        _autoForce = std::chrono::duration_cast<Clock::duration>(std::chrono::nanoseconds((long long)(1.5e9 / _eventRate)));
    }
    double getEventRate() const { return _eventRate; }

    void setSlope(const std::string &slope)
    {
        if (slope == "POS") _slopeCode = PCX_TRIGGER_POS;
        else if (slope == "NEG") _slopeCode = PCX_TRIGGER_NEG;
        else if (slope == "LEVEL") _slopeCode = PCX_TRIGGER_LEVEL;
        else throw InvalidArgumentException("WaveTrigger::setSlope(" + slope + ")", "unknown slope setting");
        _slope = slope;
    }
    std::string getSlope() const { return _slope; }

    void setMode(const std::string &mode)
    {
        if (mode != "AUTOMATIC" && mode != "SEMIAUTOMATIC" && mode != "NORMAL" && mode != "PERIODIC" && mode != "DISABLED")
            throw InvalidArgumentException("WaveTrigger::setMode(" + mode + ")", "unknown mode setting");
        _mode = mode;
        _windowTimerOn = mode == "SEMIAUTOMATIC";
        _timerOn = mode == "AUTOMATIC" || mode == "PERIODIC";
        _periodic = mode == "PERIODIC";
        _searchOn = mode == "AUTOMATIC" || mode == "SEMIAUTOMATIC" || mode == "NORMAL";
    }
    std::string getMode() const { return _mode; }

    void setLevel(const double level) { _level = level; }
    double getLevel() const { return _level; }

    void setPosition(const size_t position) { _position = position; }
    size_t getPosition() const { return _position; }

    void setLabelId(const std::string &id) { _labelId = id; }
    std::string getLabelId() const { return _labelId; }

    void setIdsList(const std::vector<std::string> &ids) { _forwardIds = std::set<std::string>(ids.begin(), ids.end()); }

    // EXTENSION (as every block of this port): the GPU that carries the block; the search handles are made again there on demand
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        dropHandles();
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer managers hand out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

    void activate()
    {
        _pointsRemaining = 0;
        _windowsRemaining = 0;
        _holdOffRemaining = 0;
        _packets.clear();
        _packets.resize(this->inputs().size());
        _lastTrigger = Clock::now();          // as if a trigger had just happened
    }

    // labels are not passed down the stream; those whose id was asked for leave as messages (WaveTrigger.cpp:406-418)
    void propagateLabels(const pcxfw::InputPort *port)
    {
        auto outPort = this->output(0);
        for (const auto &label : port->labels()) {
            if (_forwardIds.find(label.id) == _forwardIds.end()) continue;
            outPort->postMessage(label);
        }
    }

#ifndef PCX_WITH_POTHOS
    // "circular" as the reference asks for (WaveTrigger.cpp:421-424), in the memory PortBlock chooses for the edge
    pcxfw::BufferManager::Sptr getInputBufferManager(const std::string &, const std::string &domain)
    {
        if (domain == kDomain) return pcxfw::BufferManager::Sptr();
        return manager(false, "circular");
    }
#endif

    void work()
    {
        auto outPort = this->output(0);
        if (_packets.size() < this->inputs().size()) _packets.resize(this->inputs().size());

        // messages go straight through; a packet is stamped with the port it came in on (WaveTrigger.cpp:481-506)
        for (auto port : this->inputs()) {
            while (port->hasMessage()) {
                auto msg = port->popMessage();
                if (msg.type() == typeid(Packet)) {
                    auto pkt = msg.extract<Packet>();
                    pkt.metadata["index"] = Object(port->index());
                    if (pkt.payload.dtype) outPort->postMessage(std::move(pkt));
                    else logTypeError(port->name(), "packet payload");
                } else {
                    outPort->postMessage(std::move(msg));
                }
            }
            // a buffer that does not say what it holds is dropped whole
            if (port->buffer().length != 0 && !port->buffer().dtype) {
                logTypeError(port->name(), "stream buffer");
                port->consume(port->elements());
                return;
            }
        }

        if (_pointsRemaining == 0) return this->triggerWork();

        const bool firstWindow = _windowsRemaining == _numWindows - 1;
        const bool lastWindow = _windowsRemaining == 0;

        // every port that has the window ready gives it to its packet; the copies of all of them are ONE capture (below)
        const void *capIn[PCX_TRIGGER_MAX_PORTS];
        void *capOut[PCX_TRIGGER_MAX_PORTS];
        size_t capBytes[PCX_TRIGGER_MAX_PORTS], ncap = 0;
        bool allAcquired = true;
        for (auto port : this->inputs()) {
            auto &packet = _packets[port->index()];

            // done on an earlier call?
            const size_t windowsAcquired = packet.payload.elements() / (_numPoints / _numWindows);
            if (windowsAcquired + _windowsRemaining == _numWindows) {
                if (!_alignment) port->consume(port->elements());
                continue;
            }

            auto buff = port->takeBuffer();
            if (buff.elements() < _pointsRemaining) {
                port->setReserve(_pointsRemaining * buff.dtype.size());
                allAcquired = false;
                continue;
            }
            buff.length = _pointsRemaining * buff.dtype.size();

            for (auto label : port->labels()) {
                label.adjust(1, buff.dtype.size());     // bytes to elements
                if (label.index >= buff.elements()) break;
                label.index += packet.payload.elements();
                packet.labels.push_back(std::move(label));
            }

            if (_fromLevel && size_t(port->index()) == _source) {
                const auto index = _position + packet.payload.elements();
                packet.labels.emplace_back("T", Object(), index);
            }

            if (firstWindow) {
                packet.metadata["index"] = Object(port->index());
                packet.metadata["position"] = Object(_eventOffset);
                packet.metadata["level"] = Object(_level);
            }

            if (_alignment) port->consume(buff.length);
            else port->consume(port->elements());
            port->setReserve(0);

            // the window goes behind what the packet holds: page-locked host memory of the whole packet's size, made on its first window
            if (!packet.payload) {
                packet.payload = pinnedChunk(buff.dtype, _numWindows == 1 ? _pointsRemaining : _numPoints);
                packet.payload.length = 0;
            }
            if (ncap == PCX_TRIGGER_MAX_PORTS) flushCapture(capIn, capOut, capBytes, ncap);
            capIn[ncap] = buff.as<const void *>();
            capOut[ncap] = reinterpret_cast<void *>(packet.payload.getEnd());
            capBytes[ncap++] = buff.dtype.size();
            packet.payload.length += buff.length;
        }
        flushCapture(capIn, capOut, capBytes, ncap);

        if (!allAcquired) return;

        if (lastWindow) for (auto port : this->inputs()) {
            outPort->postMessage(_packets[port->index()]);
            _packets[port->index()] = Packet();
        }

        _pointsRemaining = 0;
        _holdOffRemaining = _holdOff;
        _lastTrigger = Clock::now();
    }

private:
    void triggerWork()
    {
        const auto trigPort = this->input(_source);
        const auto &trigBuff = trigPort->buffer();

        // a search needs windows left over or the event period gone by, and no hold-off running (WaveTrigger.cpp:610-611)
        const auto timePassed = Clock::now() - _lastTrigger;
        const bool searchEnabled = (_windowsRemaining > 0 || timePassed > _eventOff) && _holdOffRemaining == 0;

        size_t numElems = trigBuff.elements();
        bool allPortsReady = true;
        for (auto port : this->inputs()) {
            if (!_alignment && port != trigPort) {
                port->consume(port->elements());
                continue;
            }
            const auto &buff = port->buffer();
            numElems = std::min(numElems, buff.elements());
            if (numElems > _position + 1) continue;
            // the history of `position`, one element behind it, one more for the slope
            port->setReserve((_position + 1 + 1) * buff.dtype.size());
            allPortsReady = false;
        }
        if (!allPortsReady) return;

        bool found = false;
        _eventOffset = _position;
        _fromLevel = false;
        if (searchEnabled && _searchOn) {
            if (!_labelId.empty()) {
                for (const auto &label : trigPort->labels()) {
                    if (label.id != _labelId) continue;
                    const auto index = label.toAdjusted(1, trigBuff.dtype.size()).index;
                    if (index < _position) continue;
                    if (index >= numElems - 1) break;
                    found = true;
                    _eventOffset = index;
                    break;
                }
            } else {
                found = this->searchLevel(trigBuff, numElems, _eventOffset);
                _fromLevel = found;
            }
            if (!found && (_timerOn || (_windowTimerOn && _windowsRemaining != 0))) found = timePassed > _autoForce;
        } else if (searchEnabled && !_searchOn) {
            found = _timerOn;         // PERIODIC: as soon as the hold-off is over
        }

        size_t consumeElems = 0;
        if (found) {
            consumeElems = size_t(_eventOffset - _position);
            _eventOffset -= consumeElems;
        } else if (_holdOffRemaining != 0) {
            consumeElems = std::min(numElems, _holdOffRemaining);
            _holdOffRemaining -= consumeElems;
        } else if (_periodic) {
            consumeElems = numElems;
        } else {
            consumeElems = numElems - _position - 1;
        }

        for (auto port : this->inputs()) {
            const auto &buff = port->buffer();
            if (_alignment || trigPort == port) port->consume(consumeElems * buff.dtype.size());
        }

        if (found) {
            if (_windowsRemaining == 0) _windowsRemaining = _numWindows;
            _windowsRemaining--;
            _pointsRemaining = _numPoints / _numWindows;
            for (auto port : this->inputs()) port->setReserve(0);
            this->yield();
        }
    }

    // searchTriggerPointReal / searchTriggerPointComplex (WaveTrigger.cpp:735-771) on the device: the first pair i in
    // [position, numElems - 2] of the buffer where it lies; 24 bytes come back
    bool searchLevel(const BufferChunk &buff, const size_t numElems, double &pos)
    {
        pcx_trigger *h = handleFor(buff.dtype);
        check(pcx_trigger_set_level(h, _level), "WaveTrigger::work()");
        check(pcx_trigger_set_slope(h, _slopeCode), "WaveTrigger::work()");
        pcx_trigger_hit hit;
        check(pcx_trigger_search(h, buff.as<const void *>(), numElems, _position, &hit), "WaveTrigger::work()");
        if (!hit.found) return false;
        pos = pcx_trigger_position(&hit, _level);
        return true;
    }

    // one window from each of n buffers into its packet: a single launch
    void flushCapture(const void *const *ins, void *const *outs, const size_t *elemBytes, size_t &n)
    {
        if (n == 0) return;
        const uint64_t start = 0;
        check(pcx_trigger_capture(anyHandle(), n, ins, elemBytes, &start, 1, _pointsRemaining, outs), "WaveTrigger::work()");
        n = 0;
    }

    pcx_trigger *handleFor(const DType &dt)
    {
        auto it = _handles.find(dt.name());
        if (it != _handles.end()) return it->second;
        int scalar;
        bool cplx;
        if (!parseTriggerType(dt, scalar, cplx)) throw InvalidArgumentException("WaveTrigger::work(" + dt.toString() + ")", "unsupported type");
        OnDevice on(_device, "WaveTrigger::work()");
        pcx_trigger *h = nullptr;
        check(pcx_trigger_create(&h, scalar, cplx ? 1 : 0), "WaveTrigger::work()");
        _handles[dt.name()] = h;
        return h;
    }
    // the capture moves bytes: any handle on the block's device serves it
    pcx_trigger *anyHandle() { return _handles.empty() ? handleFor(DType("uint8")) : _handles.begin()->second; }
    void dropHandles()
    {
        for (auto &kv : _handles) pcx_trigger_destroy(kv.second);
        _handles.clear();
    }

    // (the bundled runtime has no logger: standard error)
    void logTypeError(const std::string &portName, const std::string &what)
    {
        std::fprintf(stderr, "WaveTrigger[%s] dropped %s with unspecified type\n", portName.c_str(), what.c_str());
    }

    // settings
    size_t _numPoints, _numWindows;
    double _eventRate;
    bool _alignment;
    size_t _source, _holdOff;
    Clock::duration _eventOff, _autoForce;
    std::string _slope, _mode;
    int _slopeCode;
    bool _timerOn, _windowTimerOn, _periodic, _searchOn;
    double _level;
    size_t _position;
    std::string _labelId;
    std::set<std::string> _forwardIds;

    // state
    bool _fromLevel;
    size_t _pointsRemaining, _windowsRemaining, _holdOffRemaining;
    double _eventOffset;
    Clock::time_point _lastTrigger;
    std::vector<Packet> _packets;
    std::map<std::string, pcx_trigger *> _handles;
};

pcxfw::BlockRegistry registerWaveTrigger("/comms/wave_trigger", &WaveTrigger::make);
pcxfw::BlockRegistry registerWaveTriggerOldPath("/blocks/wave_trigger", &WaveTrigger::make);

}  // namespace
