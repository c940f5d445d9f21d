// frame_plan.hpp -- the host side of /comms/preamble_framer and /comms/frame_insert: the label walk of the reference's
// two framers (digital/PreambleFramer.cpp:138-216, digital/FrameInsert.cpp:183-288) as a PLAN, and the header coder of
// digital/FrameHelper.hpp.  Plain C++: no HIP, no allocation besides the vectors of the plan; pcx_frm_api.hip, the sanitizer program of
// tests/test_framer_cpu.py and nothing else include it.
//
// The reference forwards slices of its input buffer and posts its preamble and padding buffers between them.  On the device the framed
// stream is one buffer, so the walk yields a SEGMENT TABLE for splice.hip: entries {dst, kind, src} in ascending dst, a segment ending
// where the next begins, the last entry a sentinel at the output length.  Everything is counted in elements.
//
// The walk is the reference's, its oddities included:
//   - an event at or behind the end of the input is neither handled nor used;
//   - the start id is tested before the end id (the caller classifies: an event is START when its id equals the start id);
//   - the shift of the labels grows by the insert of a start event only at the next event with a DIFFERENT index: two starts at one index
//     insert twice and shift once;
//   - an end event's head runs to index + width, clipped to the input, and its padding joins the shift before the event itself is posted.
// Two things differ:
//   - an event whose head would end in front of what is already passed on (an end event's width reached across it) has an EMPTY head: its
//     insert goes where the output stands.  The reference's unsigned difference wraps there and a buffer past its input is posted;
//   - the output has a capacity.  Events are taken in GROUPS: an event, and after it every event that lies at the same index or in front of
//     what the group has passed on.  A group is taken whole or not at all, with the element its last label sits on, so that a label that
//     was handled is also consumed.  At the first group that does not fit the call ends in front of that group's index, or at the
//     capacity if even that is too far.  A group that no empty buffer of this capacity could take is an error.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace pcx {
namespace frm {

// ---- the header of /comms/frame_insert: 58 bits, bit i of the word is the i-th symbol's bit
constexpr int kHeaderBits = 2 + (8 + 12 + 8) * 2;

// the 8-bit sum of FrameHelper.hpp: rotate right by one, then add, over id, length low, length high
inline uint8_t header_checksum(uint8_t id, uint16_t length)
{
    const uint8_t bytes[3] = {id, (uint8_t)(length & 0xff), (uint8_t)(length >> 8)};
    uint8_t acc = 0;
    for (const uint8_t b : bytes) {
        acc = (uint8_t)((acc >> 1) | ((acc & 1u) << 7));
        acc = (uint8_t)(acc + b);
    }
    return acc;
}
// Hamming(8,4) of the low four bits of x: bit k of the result is code bit k
inline uint8_t hamming84(unsigned x)
{
    const unsigned d0 = x & 1u, d1 = (x >> 1) & 1u, d2 = (x >> 2) & 1u, d3 = (x >> 3) & 1u;
    return (uint8_t)((d0 ^ d1 ^ d3) | (d0 ^ d2 ^ d3) << 1 | d0 << 2 | (d1 ^ d2 ^ d3) << 3 | d1 << 4 | d2 << 5 | d3 << 6 | (d0 ^ d1 ^ d2) << 7);
}
// time sync 0, 1; the id; TWELVE bits of the length; the checksum over all SIXTEEN
inline uint64_t header_bits(uint8_t id, uint16_t length)
{
    const uint8_t chk = header_checksum(id, length);
    const unsigned nibbles[7] = {id & 0xfu, (unsigned)id >> 4, length & 0xfu, (length >> 4) & 0xfu, (length >> 8) & 0xfu, chk & 0xfu, (unsigned)chk >> 4};
    uint64_t w = 2;
    for (int k = 0; k < 7; k++) w |= (uint64_t)hamming84(nibbles[k]) << (2 + 8 * k);
    return w;
}

// ---- the plan
enum EventKind { EV_OTHER = 0, EV_START = 1, EV_END = 2 };
enum SegKind { SEG_INPUT = 0, SEG_POOL = 1, SEG_HEADER = 2, SEG_ZERO = 3 };

struct Event {
    uint64_t index, width;
    uint32_t kind;
    uint32_t length;       // START with a header: the 16-bit length field
};
struct Segment {
    uint64_t dst;          // first output element
    uint64_t src;          // INPUT: input element; POOL: element of the sync word; HEADER: index of the frame's bit word; ZERO: 0
    uint32_t kind;
    uint32_t reserved;
};
struct Settings {
    uint64_t sync_len = 1;         // elements of the sync word: preamble symbols times symbol width
    bool header = false;           // 58 header symbols behind the sync word
    uint64_t padding = 0;
    uint8_t header_id = 0x55;
    uint64_t insert_len() const { return sync_len + (header ? (uint64_t)kHeaderBits : 0); }
};
struct Plan {
    uint64_t consumed = 0;         // input elements the call consumes
    uint64_t used_events = 0;
    uint64_t out_len = 0;
    bool cut = false;              // the capacity ended the call in front of a group
    std::vector<unsigned char> used;       // per event
    std::vector<uint64_t> insert_at;       // per used event: where its insert begins in the output (OTHER: where its label lands)
    std::vector<uint64_t> shift;           // per used event: what the block adds to the label's index
    std::vector<Segment> segs;             // ascending dst, no empty segment, the sentinel {out_len, 0, ZERO} last
    std::vector<uint64_t> headers;         // one word of header bits per START segment pair with a header
    std::string error;                     // not empty: the plan failed
};

namespace detail {
struct Walk {
    uint64_t consumed = 0, out = 0, shift = 0, need = 0, last_found = 0;
    bool found = false;
};
inline void emit(Plan &p, Walk &w, uint32_t kind, uint64_t src, uint64_t len)
{
    if (!len) return;
    p.segs.push_back(Segment{w.out, src, kind, 0});
    w.out += len;
}
inline void handle(Plan &p, Walk &w, const Settings &s, const Event &e, size_t i, uint64_t n_in)
{
    if (w.found && w.last_found != e.index) {
        w.found = false;
        w.shift += s.insert_len();
    }
    if (e.kind == EV_START) {
        const uint64_t head = e.index > w.consumed ? e.index - w.consumed : 0;
        emit(p, w, SEG_INPUT, w.consumed, head);
        w.consumed += head;
        p.insert_at[i] = w.out;
        emit(p, w, SEG_POOL, 0, s.sync_len);
        if (s.header) {
            emit(p, w, SEG_HEADER, p.headers.size(), kHeaderBits);
            p.headers.push_back(header_bits(s.header_id, (uint16_t)e.length));
        }
        w.found = true;
        w.last_found = e.index;
    } else if (e.kind == EV_END) {
        const uint64_t end = e.width > UINT64_MAX - e.index ? UINT64_MAX : e.index + e.width;
        const uint64_t head = end > w.consumed ? std::min(end - w.consumed, n_in - w.consumed) : 0;
        emit(p, w, SEG_INPUT, w.consumed, head);
        w.consumed += head;
        p.insert_at[i] = w.out;
        emit(p, w, SEG_ZERO, 0, s.padding);
        w.shift += s.padding;
    } else {
        p.insert_at[i] = e.index + w.shift;
    }
    p.shift[i] = w.shift;
    p.used[i] = 1;
    w.need = std::max(w.need, e.index + 1);
}
inline uint64_t through(const Walk &w) { return w.need > w.consumed ? w.need - w.consumed : 0; }
}  // namespace detail

// n_in input elements, room for `cap` output elements, the call's events in the order of the port (ascending index)
inline Plan plan(const Settings &s, uint64_t n_in, uint64_t cap, const Event *ev, size_t n_ev)
{
    using namespace detail;
    Plan p;
    p.used.assign(n_ev, 0);
    p.insert_at.assign(n_ev, 0);
    p.shift.assign(n_ev, 0);
    Walk w;
    uint64_t tail = 0;
    size_t i = 0;
    while (i < n_ev) {
        if (ev[i].index >= n_in) { i++; continue; }
        // the group that begins at event i, walked on a copy
        const size_t seg_mark = p.segs.size(), hdr_mark = p.headers.size();
        Walk t = w;
        size_t j = i;
        do {
            handle(p, t, s, ev[j], j, n_in);
            j++;
        } while (j < n_ev && ev[j].index < std::max(t.consumed, t.need));
        if (t.out <= cap && through(t) <= cap - t.out) {
            w = t;
            i = j;
            continue;
        }
        // it does not fit: the call ends in front of it.  What the group needs of a buffer that begins at its index:
        const uint64_t stop = std::max(ev[i].index, w.consumed);
        const uint64_t alone = (t.out - w.out) + through(t) - (stop - w.consumed);
        p.segs.resize(seg_mark);
        p.headers.resize(hdr_mark);
        for (size_t k = i; k < j; k++) p.used[k] = 0;
        if (alone > cap) {
            p.error = "framer: the inserts at index " + std::to_string(ev[i].index) + " need " + std::to_string(alone) +
                      " output elements, the output buffer holds " + std::to_string(cap);
            return p;
        }
        p.cut = true;
        tail = std::min(stop - w.consumed, cap - w.out);
        break;
    }
    if (!p.cut) tail = std::min(n_in - w.consumed, cap - w.out);
    emit(p, w, SEG_INPUT, w.consumed, tail);
    p.consumed = w.consumed + tail;
    p.out_len = w.out;
    for (const unsigned char u : p.used) p.used_events += u;
    p.segs.push_back(Segment{p.out_len, 0, SEG_ZERO, 0});
    return p;
}

}  // namespace frm
}  // namespace pcx
