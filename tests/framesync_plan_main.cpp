// Stand-alone program around frame_sync_plan.hpp (the host side of /comms/frame_sync) for tests/test_framesync_cpu.py, which builds
// it with the address and undefined-behaviour sanitizers.  One request per line on the standard input, one answer per line:
//   hdr <word> <expected id>                 -> id length checksum error accepted
//   found <mode> <dw> <F> <phase id?> <start id?> <end id?> <frame offset> <first bit> <deltaFc> <phaseOff> <length>
//                                            -> consumed remaining phase phase_inc n, then per label: kind index width length value
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "frame_sync_plan.hpp"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "hdr") {
            uint64_t word;
            unsigned id;
            in >> word >> id;
            const pcx::fsy::Header h = pcx::fsy::decode_header(word);
            std::printf("%u %u %u %d %d\n", (unsigned)h.id, (unsigned)h.length, (unsigned)h.chksum, h.error ? 1 : 0, pcx::fsy::header_accepted(h, (uint8_t)id) ? 1 : 0);
        } else if (what == "found") {
            pcx::fsy::Settings s;
            int p, st, e;
            int64_t off;
            uint64_t first;
            double dfc, poff;
            unsigned length;
            in >> s.mode >> s.dw >> s.F >> p >> st >> e >> off >> first >> dfc >> poff >> length;
            s.phase_id = p != 0;
            s.start_id = st != 0;
            s.end_id = e != 0;
            const pcx::fsy::Found f = pcx::fsy::frame_found(s, off, first, dfc, poff, (uint16_t)length);
            std::printf("%" PRIu64 " %" PRIu64 " %.17g %.17g %u", f.consumed, f.remaining, f.phase, f.phase_inc, f.n_labels);
            for (unsigned k = 0; k < f.n_labels; k++)
                std::printf(" %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %.17g", f.labels[k].kind, f.labels[k].index, f.labels[k].width, f.labels[k].length, f.labels[k].value);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
