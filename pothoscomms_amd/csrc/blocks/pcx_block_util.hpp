// pcx_block_util.hpp -- helpers that the module sources (comms_blocks.cpp, filter_blocks.cpp) share.  They register nothing: every
// registerCall line stays in the source that holds the block's description.  Built against pcx_framework.hpp (PothosCore when
// -DPCX_WITH_POTHOS, the bundled runtime otherwise).
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

}  // namespace pcxblk
