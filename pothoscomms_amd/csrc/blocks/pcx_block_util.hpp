// pcx_block_util.hpp -- what the module sources (comms_blocks.cpp and every *_blocks.cpp) share: the element-type parser, the
// status check, the device scope, and PortBlock, the base of the blocks outside comms_blocks.cpp (the device a block is on, its
// port slabs and their buffer managers).  Nothing here registers a call: every registerCall line stays in the source that holds the
// block's description.  Built against pcx_framework.hpp (PothosCore when -DPCX_WITH_POTHOS, the bundled runtime otherwise).
#pragma once
#include <cstddef>
#include <string>

#include "pcx.h"
#include "pcx_framework.hpp"

namespace pcxblk {

// DType element name -> (pcx_scalar, complex?)
inline bool parseElemType(const pcxfw::DType &dt, int &scalar, bool &cplx)
{
    std::string n = pcxfw::DType::fromDType(dt, 1).name();
    cplx = n.compare(0, 8, "complex_") == 0;
    if (cplx) n = n.substr(8);
    if (n == "float64") scalar = PCX_F64;
    else if (n == "float32") scalar = PCX_F32;
    else if (n == "int64") scalar = PCX_I64;
    else if (n == "int32") scalar = PCX_I32;
    else if (n == "int16") scalar = PCX_I16;
    else if (n == "int8") scalar = PCX_I8;
    else return false;
    return true;
}
// ABI status -> the exception type the reference would throw at that point
inline void check(int rc, const std::string &where)
{
    if (rc == PCX_OK) return;
    const std::string msg = pcx_last_error();
    if (rc == PCX_ERR_ARG) throw pcxfw::InvalidArgumentException(where, msg);
    throw pcxfw::Exception(where, msg);
}

// bounds of a block's port-slab setting (setPortSlabBytes); the default is comms_blocks.cpp's kPortSlabBytes
constexpr size_t kPortSlabMin = 64u << 10, kPortSlabMax = 1u << 30;
// the port domain of this port's blocks (comms_blocks.cpp: the edges between two of them live in device memory)
constexpr const char *kDomain = "pcx-hip";

// the calling thread's current device for the length of a scope (the C ABI binds a handle to the device current when it is
// CREATED and runs the stateless maps on the device current when they are CALLED, include/pcx.h)
class OnDevice {
public:
    explicit OnDevice(int device, const char *where = "DeviceBlock") : _prev(-1)
    {
        int cur = -1;
        if (device < 0 || pcx_get_device(&cur) != PCX_OK || cur == device) return;
        check(pcx_set_device(device), where);
        _prev = cur;
    }
    ~OnDevice() { if (_prev >= 0) (void)pcx_set_device(_prev); }
    OnDevice(const OnDevice &) = delete;
    OnDevice &operator=(const OnDevice &) = delete;

private:
    int _prev;
};

// What the blocks of the further modules share as every block of this port does: the device, the port slabs and their managers.
// `who` is the block's name as its exceptions spell it, `slabBytes` the module's kPortSlabBytes.  A block keeps the part of
// setDevice() that is its own (a fresh handle there, the settings pushed again, the swap) and one-line public getDevice(),
// setPortSlabBytes() and getPortSlabBytes(): registerCall() cannot deduce a method that lives in a base class.
class PortBlock : public pcxfw::Block {
public:
    PortBlock(const std::string &who, size_t slabBytes) : _who(who), _device(-1), _slabBytes(slabBytes)
    {
        int cur = -1;
        if (pcx_get_device(&cur) == PCX_OK) _device = cur;
    }
#ifndef PCX_WITH_POTHOS
    // (bundled runtime) page-locked slabs towards host blocks, device slabs between two blocks of this port
    pcxfw::BufferManager::Sptr getInputBufferManager(const std::string &, const std::string &domain)
    {
        if (domain == kDomain) return pcxfw::BufferManager::Sptr();
        return manager(false);
    }
    pcxfw::BufferManager::Sptr getOutputBufferManager(const std::string &, const std::string &domain)
    {
        const std::string where = _who + "::getOutputBufferManager()";
        OnDevice on(_device, where.c_str());
        return manager(domain == kDomain);
    }
#endif

protected:
    // the device a setDevice() asks for, checked against what the process sees
    int checkedDevice(const size_t device) const
    {
        int n = 0;
        check(pcx_device_count(&n), _who + "::setDevice()");
        if (device >= (size_t)n)
            throw pcxfw::InvalidArgumentException(_who + "::setDevice(" + std::to_string(device) + ")", "the process sees " + std::to_string(n) + " device(s)");
        return (int)device;
    }
    void checkedSlab(const size_t bytes)
    {
        if (bytes < kPortSlabMin || bytes > kPortSlabMax)
            throw pcxfw::InvalidArgumentException(_who + "::setPortSlabBytes(" + std::to_string(bytes) + ")", "64 KiB ... 1 GiB");
        _slabBytes = bytes;
    }
#ifndef PCX_WITH_POTHOS
    pcxfw::BufferManager::Sptr manager(bool device, const std::string &name = "generic") const
    {
        pcxfw::BufferManagerArgs args;
        args.bufferSize = _slabBytes;
        args.numBuffers = 4;
        if (device) args.device = true;
        else args.pinned = true;
        return pcxfw::BufferManager::make(name, args);
    }
#endif
    const std::string _who;
    int _device;
    size_t _slabBytes;
};

}  // namespace pcxblk
