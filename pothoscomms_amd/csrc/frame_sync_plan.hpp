// frame_sync_plan.hpp -- the host side of /comms/frame_sync: what digital/FrameSync.cpp:533-587 does once the device has
// handed back the 58 header bits and the sampling offset of the first one -- the Hamming(8,4) decoder and the checks of
// digital/FrameHelper.hpp, the labels, the payload offset and the backing up of the DEBUG mode.  Plain C++: no HIP, no allocation;
// pcx_fsync_api.hip, the sanitizer program of tests/test_framesync_cpu.py and nothing else include it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "frame_plan.hpp"

namespace pcx {
namespace fsy {

enum Mode { MODE_RAW = 0, MODE_PHASE = 1, MODE_TIMING = 2, MODE_DEBUG = 3 };
enum LabelKind { LABEL_PHASE_OFFSET = 0, LABEL_FRAME_START = 1, LABEL_FRAME_END = 2 };

struct Header {
    uint8_t id = 0;
    uint16_t length = 0;
    uint8_t chksum = 0;
    bool error = false;
};

// decodeHamming84: code bit k in bit k of `code`; one flipped bit is corrected, two set `error`
inline unsigned hamming84_decode(unsigned code, bool &error)
{
    unsigned b[8];
    for (int k = 0; k < 8; k++) b[k] = (code >> k) & 1u;
    const unsigned p0 = (b[0] + b[2] + b[4] + b[6]) & 1u, p1 = (b[1] + b[2] + b[5] + b[6]) & 1u, p2 = (b[3] + b[4] + b[5] + b[6]) & 1u;
    const unsigned p3 = (b[0] + b[1] + b[2] + b[3] + b[4] + b[5] + b[6] + b[7]) & 1u;
    const unsigned parity = p0 | p1 << 1 | p2 << 2 | p3 << 3;
    if (parity >= 1 && parity <= 7) error = true;
    else if (parity == 8) b[7] ^= 1u;
    else if (parity >= 9) b[parity - 9] ^= 1u;
    return b[2] | b[4] << 1 | b[5] << 2 | b[6] << 3;
}

// decodeHeaderWord: bit i of `bits` is the i-th header symbol's bit
inline Header decode_header(uint64_t bits)
{
    Header h;
    unsigned nib[7];
    for (int k = 0; k < 7; k++) nib[k] = hamming84_decode((unsigned)(bits >> (2 + 8 * k)) & 0xffu, h.error);
    h.id = (uint8_t)(nib[0] | nib[1] << 4);
    h.length = (uint16_t)(nib[2] | nib[3] << 4 | nib[4] << 8);
    h.chksum = (uint8_t)(nib[5] | nib[6] << 4);
    return h;
}

// FrameSync.cpp:533-536
inline bool header_accepted(const Header &h, uint8_t header_id)
{
    if (h.error) return false;
    if (h.chksum != frm::header_checksum(h.id, h.length)) return false;
    if (h.id != header_id) return false;
    return h.length != 0;
}

struct Settings {
    uint64_t dw = 4, F = 80 + 58 * 4;
    int mode = MODE_RAW;
    bool phase_id = false, start_id = true, end_id = false;       // which label ids are not empty
};
struct Label {
    uint32_t kind = 0;
    uint64_t index = 0, width = 0, length = 0;
    double value = 0;
};
struct Found {
    uint64_t consumed = 0, remaining = 0;
    double phase = 0, phase_inc = 0;
    Label labels[3];
    unsigned n_labels = 0;
};

// FrameSync.cpp:537-586: a valid header `length` at frame_off (elements from the call's first; it may lie in front of it), its first bit
// sampled first_bit elements behind that
inline Found frame_found(const Settings &s, int64_t frame_off, uint64_t first_bit, double delta_fc, double phase_off, uint16_t length)
{
    Found f;
    const uint64_t label_width = s.mode == MODE_TIMING ? 1 : s.dw;
    uint64_t payload_off = (uint64_t)frame_off + first_bit + (uint64_t)frm::kHeaderBits * s.dw + label_width / 2;
    uint64_t label_start = 0, label_end = ((uint64_t)length - 1) * label_width;
    f.remaining = (uint64_t)length * s.dw;
    f.phase_inc = delta_fc;
    f.phase = phase_off + f.phase_inc * (double)s.F;
    if (s.mode == MODE_DEBUG) {
        const uint64_t backup = std::min(payload_off, s.F);
        label_start += backup;
        label_end += backup;
        f.phase -= f.phase_inc * (double)backup;
        f.remaining += backup;
        payload_off -= backup;
    }
    auto post = [&](uint32_t kind, uint64_t index, double value) {
        Label &l = f.labels[f.n_labels++];
        l.kind = kind;
        l.index = index;
        l.width = label_width;
        l.length = length;
        l.value = value;
    };
    if (s.phase_id) post(LABEL_PHASE_OFFSET, label_start, f.phase);
    if (s.start_id) post(LABEL_FRAME_START, label_start, 0);
    if (s.end_id) post(LABEL_FRAME_END, label_end, 0);
    f.consumed = payload_off;
    return f;
}

}  // namespace fsy
}  // namespace pcx
