// waveform_blocks.cpp -- the ninth module of this port: the two blocks of the reference's waveform/ directory, the ones that produce a
// stream, libpcx_waveform_blocks.so (with the runner ABI of include/pcx_blocks.h linked in).  In a PothosComms build this source is the
// WaveformBlocks module.
//
//   /comms/waveform_source, /blocks/waveform_source       waveform/WaveformSource.cpp:68-293
//   /comms/noise_source, /blocks/noise_source             waveform/NoiseSource.cpp:71-289
//
// Both keep the reference's shape: the settings live in the block, the table is built on the host (pcx_waveform_table, pcx_noise_table)
// only while the block is active and by activate(), and work() walks it from the carried index, on the device (pcx_source).
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

using namespace pcxblk;     // check, OnDevice, kDomain, the port-slab bounds, PortBlock (pcx_block_util.hpp)

// the default port slab of every block of this port (comms_blocks.cpp's kPortSlabBytes; tests/test_source_cpu.py keeps them equal)
constexpr size_t kPortSlabBytes = 64u << 20;

// what the two blocks share: the device walk of a table (pcx_source), its element type and the extension calls
class SourceBlock : public PortBlock {
public:
    SourceBlock(const std::string &who, const DType &dtype, int scalar, bool cplx)
        : PortBlock(who, kPortSlabBytes), _scalar(scalar), _cplx(cplx), _es(dtype.size()), _h(nullptr)
    {
        check(pcx_source_create(scalar, cplx ? 1 : 0, &_h), _who + "()");
        Block::setupOutput(0, dtype, kDomain);
    }
    ~SourceBlock() { pcx_source_destroy(_h); }

    // EXTENSION (as every block of this port): the GPU that carries the block; the handle is created again there with the carried
    // index, and with the table when the block is active
    void setDevice(const size_t device)
    {
        const int d = checkedDevice(device);
        const std::string where = _who + "::setDevice()";
        OnDevice on(d, where.c_str());
        uint64_t index = 0;
        check(pcx_source_get_index(_h, &index), where);
        pcx_source *fresh = nullptr;
        check(pcx_source_create(_scalar, _cplx ? 1 : 0, &fresh), where);
        int rc = pcx_source_set_index(fresh, index);
        if (rc == PCX_OK && !_table.empty()) rc = pcx_source_set_table(fresh, _table.data(), _table.size() / _es, _step);
        if (rc != PCX_OK) {
            pcx_source_destroy(fresh);      // (leaves the library's message as it is)
            check(rc, where);
        }
        pcx_source_destroy(_h);
        _h = fresh;
        _device = d;
    }
    size_t getDevice() const { return _device < 0 ? 0 : (size_t)_device; }
    // EXTENSION: the size of the port slabs the block's buffer manager hands out (an initializer)
    void setPortSlabBytes(const size_t bytes) { checkedSlab(bytes); }
    size_t getPortSlabBytes() const { return _slabBytes; }

protected:
    // the table the next work() walks
    void pushTable(uint64_t step, const std::string &where)
    {
        _step = step;
        check(pcx_source_set_table(_h, _table.data(), _table.size() / _es, step), where);
    }
    // work (WaveformSource.cpp:98-108, NoiseSource.cpp:105-130): all the space offered is filled and produced
    void fill(const std::string &where)
    {
        auto outPort = this->output(0);
        const size_t n = outPort->elements();
        if (n == 0) return;
        check(pcx_source_generate(_h, outPort->buffer().template as<void *>(), n), where);
        outPort->produce(n);
    }
    const int _scalar;
    const bool _cplx;
    const size_t _es;
    pcx_source *_h;
    std::vector<unsigned char> _table;      // as it was built last; empty until the block was active once
    uint64_t _step = 0;
};

/***********************************************************************
 * |PothosDoc Waveform Source
 *
 * Produces simple cyclical waveforms on the GPU.  With a complex data type the real and the imaginary component
 * of the output are 90 degrees out of phase.  The samples are entries of a wave table that the block walks with
 * a fixed step, so every one of them is what the host block would have produced.
 *
 * |category /Sources
 * |category /Waveforms
 * |keywords cosine sine ramp square waveform source signal
 * |alias /blocks/waveform_source
 *
 * |param dtype[Data Type] Element type of the output stream.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param wave[Wave Type] Shape of one cycle of the output.
 * |option [Constant] "CONST"
 * |option [Sinusoid] "SINE"
 * |option [Ramp] "RAMP"
 * |option [Square] "SQUARE"
 * |default "SINE"
 *
 * |param rate[Sample Rate] How many output samples make up one second.
 * |units samples/sec
 * |default 1.0
 *
 * |param freq[Frequency] Cycles per second, between minus and plus half the sample rate.
 * |units Hz
 * |default 0.1
 *
 * |param ampl[Amplitude] Complex factor every entry of the wave table is multiplied by.
 * |default 1.0
 *
 * |param offset Complex value added to every entry once it has been multiplied by the amplitude.
 * |default 0.0
 * |preview valid
 *
 * |param res[Resolution] Frequency step in Hz the wave table must be able to resolve, or zero.
 * At zero the table grows with falling frequency until one sample advances it by 16 entries or it holds a million entries.
 * Any other value takes the place of the frequency in that rule, so the table keeps its size when the frequency changes.
 * |units Hz
 * |default 0.0
 * |preview valid
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
 * |factory /comms/waveform_source(dtype)
 * |setter setSampleRate(rate)
 * |setter setWaveform(wave)
 * |setter setOffset(offset)
 * |setter setAmplitude(ampl)
 * |setter setFrequency(freq)
 * |setter setResolution(res)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class WaveformSource : public SourceBlock {
public:
    WaveformSource(const DType &dtype, int scalar, bool cplx)
        : SourceBlock("WaveformSource", dtype, scalar, cplx), _rate(1.0), _freq(0.0), _res(0.0), _offset(0.0), _scalarAmpl(1.0), _wave("CONST")
    {
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setWaveform));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getWaveform));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setOffset));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getOffset));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setAmplitude));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getAmplitude));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setFrequency));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getFrequency));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setSampleRate));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getSampleRate));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setResolution));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getResolution));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(WaveformSource, getPortSlabBytes));
    }

    void activate() { this->updateTable(); }
    void work() { this->fill("WaveformSource::work()"); }

    // the setters and getters of :110-174: the value is kept, then the table follows while the block is active
    void setWaveform(const std::string &wave) { _wave = wave; this->updateTable(); }
    std::string getWaveform() { return _wave; }
    void setOffset(const std::complex<double> &offset) { _offset = offset; this->updateTable(); }
    std::complex<double> getOffset() { return _offset; }
    void setAmplitude(const std::complex<double> &scalar) { _scalarAmpl = scalar; this->updateTable(); }
    std::complex<double> getAmplitude() { return _scalarAmpl; }
    void setFrequency(const double &freq) { _freq = freq; this->updateTable(); }
    double getFrequency() { return _freq; }
    void setSampleRate(const double &rate) { _rate = rate; this->updateTable(); }
    double getSampleRate() { return _rate; }
    void setResolution(const double &res) { _res = res; this->updateTable(); }
    double getResolution() { return _res; }

    void setDevice(const size_t device) { SourceBlock::setDevice(device); }
    size_t getDevice() const { return SourceBlock::getDevice(); }
    void setPortSlabBytes(const size_t bytes) { SourceBlock::setPortSlabBytes(bytes); }
    size_t getPortSlabBytes() const { return SourceBlock::getPortSlabBytes(); }

private:
    // updateTable (:178-247).  The carried index is left alone: it enters a table of another size as _index does.
    void updateTable()
    {
        if (!this->isActive()) return;
        const int wave = _wave == "CONST" ? PCX_WAVE_CONST : _wave == "SINE" ? PCX_WAVE_SINE : _wave == "RAMP" ? PCX_WAVE_RAMP
                         : _wave == "SQUARE" ? PCX_WAVE_SQUARE : -1;
        // the reference's two throws, in its order: the step first (from updateTable()), then the wave (from setWaveform(<wave>))
        size_t entries = 0;
        uint64_t step = 0;
        check(pcx_waveform_table(_scalar, _cplx, PCX_WAVE_CONST, _rate, _freq, _res, 0, 0, 0, 0, nullptr, 0, &entries, &step), "WaveformSource::updateTable()");
        if (wave < 0) throw InvalidArgumentException("WaveformSource::setWaveform(" + _wave + ")", "unknown waveform setting");
        _table.resize(entries * _es);
        check(pcx_waveform_table(_scalar, _cplx, wave, _rate, _freq, _res, _scalarAmpl.real(), _scalarAmpl.imag(), _offset.real(), _offset.imag(),
                                 _table.data(), entries, &entries, &step),
              "WaveformSource::updateTable()");
        this->pushTable(step, "WaveformSource::updateTable()");
    }

    double _rate, _freq, _res;
    std::complex<double> _offset, _scalarAmpl;
    std::string _wave;
};

/***********************************************************************
 * |PothosDoc Noise Source
 *
 * Produces pseudorandom noise patterns on the GPU.  With a complex data type the real and the imaginary component
 * are two independent channels.  The block draws a pool of 4096 samples whenever a setting changes and reads
 * it from a random position at every call, as the host block does in its fast mode (the only one it has).
 * The generator is seeded from the system's entropy source; the call setSeed(seed) seeds it with a number instead.
 *
 * |category /Sources
 * |category /Waveforms
 * |category /Random
 * |keywords noise random source pseudorandom gaussian
 * |alias /blocks/noise_source
 *
 * |param dtype[Data Type] Element type of the output stream.
 * |widget DTypeChooser(float=1,cfloat=1,int=1,cint=1)
 * |default "complex_float32"
 * |preview disable
 *
 * |param wave[Wave Type] Distribution the pool of samples is drawn from.
 * |option [Uniform] "UNIFORM"
 * |option [Normal] "NORMAL"
 * |option [Laplace] "LAPLACE"
 * |option [Poisson] "POISSON"
 * |default "NORMAL"
 *
 * |param ampl[Amplitude] Complex factor every drawn sample is multiplied by.
 * |default 1.0
 *
 * |param offset Complex value added to every sample once it has been multiplied by the amplitude.
 * |default 0.0
 * |preview valid
 *
 * |param mean Centre of the distribution, whichever one is chosen.
 * |default 0.0
 * |preview valid
 *
 * |param b Width of the distribution.  Uniform samples lie within b of the mean on either side, for normal samples b is
 * the standard deviation, and for Laplace samples it is the scale of the two exponential tails.  Poisson samples ignore it.
 * |default 1.0
 *
 * |param fast[Fast] Whether samples come from the pool of 4096 or are drawn one by one.  No call changes it, here as in the host block, so the pool is always used.
 * |option [Enabled] true
 * |option [Disabled] false
 * |default true
 * |preview invalid
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
 * |factory /comms/noise_source(dtype)
 * |setter setWaveform(wave)
 * |setter setOffset(offset)
 * |setter setAmplitude(ampl)
 * |setter setMean(mean)
 * |setter setB(b)
 * |initializer setPortSlabBytes(portSlabBytes)
 * |initializer setDevice(device)
 **********************************************************************/
class NoiseSource : public SourceBlock {
public:
    NoiseSource(const DType &dtype, int scalar, bool cplx)
        : SourceBlock("NoiseSource", dtype, scalar, cplx), _offset(0.0), _scalarAmpl(1.0), _wave("NORMAL"), _mean(0.0), _b(1.0), _gen(nullptr)
    {
        check(pcx_noise_create(0, 0, &_gen), "NoiseSource()");      // _gen(_rd()), :84
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setWaveform));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, getWaveform));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setOffset));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, getOffset));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setAmplitude));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, getAmplitude));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setMean));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, getMean));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setB));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, getB));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setSeed));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setDevice));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, getDevice));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, setPortSlabBytes));
        this->registerCall(this, PCX_FCN_TUPLE(NoiseSource, getPortSlabBytes));
    }
    ~NoiseSource() { pcx_noise_destroy(_gen); }

    void activate() { this->updateTable(); }
    // work (:105-130), the fast branch: the index moves on by a draw (on every call, an empty one included), then the table is walked from it
    void work()
    {
        size_t draw = 0;
        check(pcx_noise_next_offset(_gen, &draw), "NoiseSource::work()");
        uint64_t index = 0;
        check(pcx_source_get_index(_h, &index), "NoiseSource::work()");
        check(pcx_source_set_index(_h, index + draw), "NoiseSource::work()");
        this->fill("NoiseSource::work()");
    }

    // the setters and getters of :132-185
    void setWaveform(const std::string &wave) { _wave = wave; this->updateTable(); }
    std::string getWaveform() { return _wave; }
    void setOffset(const std::complex<double> &offset) { _offset = offset; this->updateTable(); }
    std::complex<double> getOffset() const { return _offset; }
    void setAmplitude(const std::complex<double> &scalar) { _scalarAmpl = scalar; this->updateTable(); }
    std::complex<double> getAmplitude() const { return _scalarAmpl; }
    void setMean(const double mean) { _mean = mean; this->updateTable(); }
    double getMean() const { return _mean; }
    void setB(const double b) { _b = b; this->updateTable(); }
    double getB() const { return _b; }

    // EXTENSION: a seed for the generator in place of std::random_device's, so that a stream can be reproduced; the table follows
    // while the block is active
    void setSeed(const size_t seed)
    {
        pcx_noise *fresh = nullptr;
        check(pcx_noise_create(1, (uint32_t)seed, &fresh), "NoiseSource::setSeed()");
        pcx_noise_destroy(_gen);
        _gen = fresh;
        this->updateTable();
    }
    void setDevice(const size_t device) { SourceBlock::setDevice(device); }
    size_t getDevice() const { return SourceBlock::getDevice(); }
    void setPortSlabBytes(const size_t bytes) { SourceBlock::setPortSlabBytes(bytes); }
    size_t getPortSlabBytes() const { return SourceBlock::getPortSlabBytes(); }

private:
    // updateTable (:188-225)
    void updateTable()
    {
        if (!this->isActive()) return;
        const int wave = _wave == "UNIFORM" ? PCX_NOISE_UNIFORM : _wave == "NORMAL" ? PCX_NOISE_NORMAL : _wave == "LAPLACE" ? PCX_NOISE_LAPLACE
                         : _wave == "POISSON" ? PCX_NOISE_POISSON : -1;
        if (wave < 0) throw InvalidArgumentException("NoiseSource::setWaveform(" + _wave + ")", "unknown waveform setting");
        _table.resize(PCX_NOISE_ENTRIES * _es);
        check(pcx_noise_table(_gen, _scalar, _cplx, wave, _mean, _b, _scalarAmpl.real(), _scalarAmpl.imag(), _offset.real(), _offset.imag(), _table.data()),
              "NoiseSource::updateTable()");
        this->pushTable(1, "NoiseSource::updateTable()");
    }

    std::complex<double> _offset, _scalarAmpl;
    std::string _wave;
    double _mean, _b;
    pcx_noise *_gen;
};

Block *waveformSourceFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) return new WaveformSource(dtype, scalar, cplx);
    throw InvalidArgumentException("waveformSourceFactory(" + dtype.toString() + ")", "unsupported type");
}
Block *noiseSourceFactory(const DType &dtype)
{
    int scalar;
    bool cplx;
    if (parseElemType(dtype, scalar, cplx) && dtype.dimension() == 1) return new NoiseSource(dtype, scalar, cplx);
    throw InvalidArgumentException("noiseSourceFactory(" + dtype.toString() + ")", "unsupported type");
}
pcxfw::BlockRegistry registerWaveformSource("/comms/waveform_source", &waveformSourceFactory);
pcxfw::BlockRegistry registerWaveformSourceOldPath("/blocks/waveform_source", &waveformSourceFactory);
pcxfw::BlockRegistry registerNoiseSource("/comms/noise_source", &noiseSourceFactory);
pcxfw::BlockRegistry registerNoiseSourceOldPath("/blocks/noise_source", &noiseSourceFactory);

}  // namespace
