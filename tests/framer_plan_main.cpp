// framer_plan_main.cpp -- a stand-alone program over pothoscomms_amd/csrc/frame_plan.hpp for tests/test_framer_cpu.py, which compiles it
// with -fsanitize=address,undefined and runs it as a child process.  It reads cases from its standard input, one per line:
//     n_in cap sync_len header padding n_events  then per event: index width kind length
// plans each, EXECUTES the segment table on real arrays of exactly n_in input and out_len output elements (so that a segment that
// reaches outside either is an error of the sanitizer, not a wrong number), checks the invariants of a plan and prints
//     consumed out_len cut used_events | used... | insert_at... | shift... | a digest of the output
// or "error <message>".  "random SEED COUNT" runs COUNT seeded random label sets through the same checks and prints one line.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "frame_plan.hpp"

using namespace pcx::frm;

static void fail(const char *what)
{
    std::printf("INVARIANT %s\n", what);
    std::exit(2);
}

// the output as element codes: input element i -> i + 1, sync word element j -> -(j + 1), header bit -> 2000000 + bit, padding -> 0
static std::vector<long long> execute(const Settings &s, uint64_t n_in, const Plan &p)
{
    std::vector<long long> in(n_in), pool(s.sync_len), out(p.out_len, -999);
    for (uint64_t i = 0; i < n_in; i++) in[i] = (long long)i + 1;
    for (uint64_t j = 0; j < s.sync_len; j++) pool[j] = -(long long)j - 1;
    for (size_t k = 0; k + 1 < p.segs.size(); k++) {
        const Segment &g = p.segs[k];
        const uint64_t len = p.segs[k + 1].dst - g.dst;
        for (uint64_t e = 0; e < len; e++) {
            long long v = 0;
            if (g.kind == SEG_INPUT) v = in.at(g.src + e);
            else if (g.kind == SEG_POOL) v = pool.at(g.src + e);
            else if (g.kind == SEG_HEADER) {
                if (e >= (uint64_t)kHeaderBits) fail("a header segment longer than the header");
                v = 2000000 + (long long)((p.headers.at(g.src) >> e) & 1u);
            }
            out.at(g.dst + e) = v;
        }
    }
    return out;
}

static void check(uint64_t n_in, uint64_t cap, const std::vector<Event> &ev, const Plan &p, const std::vector<long long> &out)
{
    if (p.consumed > n_in) fail("consumed more than the input");
    if (p.out_len > cap) fail("produced more than the capacity");
    if (p.segs.empty() || p.segs.back().dst != p.out_len) fail("no sentinel at the output length");
    if (!p.segs.empty() && p.out_len && p.segs.front().dst != 0) fail("the table does not begin at 0");
    for (size_t k = 0; k + 1 < p.segs.size(); k++)
        if (p.segs[k].dst >= p.segs[k + 1].dst) fail("dst not strictly ascending");
    // the input elements appear once each, in order, and are exactly the consumed ones
    long long next = 1;
    for (const long long v : out) {
        if (v == -999) fail("an output element no segment wrote");
        if (v > 0 && v < 2000000) {
            if (v != next) fail("input elements out of order");
            next++;
        }
    }
    if ((uint64_t)(next - 1) != p.consumed) fail("consumed differs from the input elements in the output");
    uint64_t used = 0;
    for (size_t i = 0; i < ev.size(); i++) {
        if (!p.used[i]) continue;
        used++;
        if (ev[i].index >= p.consumed) fail("a handled label on an element that is not consumed");
        if (ev[i].kind != EV_OTHER && p.insert_at[i] > p.out_len) fail("an insert behind the output");
    }
    if (used != p.used_events) fail("used_events");
}

static void print(const Plan &p, const std::vector<long long> &out)
{
    std::printf("%llu %llu %d %llu |", (unsigned long long)p.consumed, (unsigned long long)p.out_len, p.cut ? 1 : 0, (unsigned long long)p.used_events);
    for (const unsigned char u : p.used) std::printf(" %d", (int)u);
    std::printf(" |");
    for (size_t i = 0; i < p.used.size(); i++) std::printf(" %llu", (unsigned long long)(p.used[i] ? p.insert_at[i] : 0));
    std::printf(" |");
    for (size_t i = 0; i < p.used.size(); i++) std::printf(" %llu", (unsigned long long)(p.used[i] ? p.shift[i] : 0));
    unsigned long long digest = 1469598103934665603ull;
    for (const long long v : out) digest = (digest ^ (unsigned long long)v) * 1099511628211ull;
    std::printf(" | %llu\n", digest);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string first;
        if (!(is >> first)) continue;
        if (first == "random") {
            unsigned seed = 0;
            int count = 0;
            is >> seed >> count;
            std::mt19937_64 rng(seed);
            unsigned long long plans = 0, errors = 0, cuts = 0;
            for (int c = 0; c < count; c++) {
                Settings s;
                s.sync_len = 1 + rng() % 40;
                s.header = rng() % 3 == 0;
                s.padding = rng() % 4 ? rng() % 20 : 0;
                s.header_id = (uint8_t)rng();
                const uint64_t n_in = rng() % 200;
                std::vector<Event> ev(rng() % 12);
                uint64_t at = 0;
                for (Event &e : ev) {
                    at += rng() % 3 ? rng() % 40 : 0;
                    e.index = at;
                    e.width = rng() % 5 ? 1 : rng() % 60;
                    if (rng() % 50 == 0) e.width = UINT64_MAX - rng() % 3;
                    e.kind = (uint32_t)(rng() % 3);
                    e.length = (uint32_t)(rng() & 0xffff);
                }
                const uint64_t cap = rng() % 4 ? rng() % 600 : n_in + ev.size() * (s.insert_len() + s.padding);
                const Plan p = plan(s, n_in, cap, ev.data(), ev.size());
                plans++;
                if (!p.error.empty()) { errors++; continue; }
                cuts += p.cut;
                check(n_in, cap, ev, p, execute(s, n_in, p));
            }
            std::printf("random %llu plans, %llu errors, %llu cuts\n", plans, errors, cuts);
            continue;
        }
        Settings s;
        uint64_t n_in = std::stoull(first), cap = 0;
        int header = 0;
        size_t n_ev = 0;
        is >> cap >> s.sync_len >> header >> s.padding >> n_ev;
        s.header = header != 0;
        std::vector<Event> ev(n_ev);
        for (Event &e : ev) is >> e.index >> e.width >> e.kind >> e.length;
        if (!is) fail("a malformed case");
        const Plan p = plan(s, n_in, cap, ev.data(), ev.size());
        if (!p.error.empty()) {
            std::printf("error %s\n", p.error.c_str());
            continue;
        }
        const std::vector<long long> out = execute(s, n_in, p);
        check(n_in, cap, ev, p, out);
        print(p, out);
    }
    return 0;
}
