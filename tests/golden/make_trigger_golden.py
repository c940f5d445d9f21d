"""Writes tests/golden/trigger.npz: what /comms/wave_trigger of the reference does, call by call, on the cases of tests/trigger_model.py.

Run where a C++ compiler and the reference tree are.  A driver of this project's own (DRIVER below) is written into a temporary
directory.  It includes utility/WaveTrigger.cpp BY PATH from the reference tree, is compiled with the oracle's flags against the stand-in
headers under tests/golden/standin_trigger, and runs the block's own work() and propagateLabels().  Nothing compiled is kept and no
text of the reference is kept: the file holds parameters, streams and recorded outputs only.  No test reads the reference tree.

The driver does what trigger_model.run_calls does: the settings, activate(), then call after call the case's events (a setter, a message
queued on an input, another type planted on a port), every port offered feed[min(k, len - 1)] elements behind what it has consumed with
the labels that lie on them (in bytes, as on a port without a type), work(), propagateLabels() on the labels inside what was consumed.
Per call it prints what every port consumed and reserved, whether the block yielded, and every message on the output: a packet's
metadata (position and level as raw bits), type, bytes and labels, or a label.

Per case the file holds the streams, the calls as JSON and the payload bytes.  The maker asserts that the model agrees with every
recorded call.

    python tests/golden/make_trigger_golden.py [--reference /root/reference] [--out tests/golden/trigger.npz]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import trigger_model as M  # noqa: E402

DRIVER = r"""
// driver <cfg.txt>: the calls of one case (the format: main below)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include <Pothos/Framework.hpp>
#define private public
#include "utility/WaveTrigger.cpp"
#undef private

struct Event { size_t call; std::string type, name, kind, sval; size_t port, u; double d; std::vector<std::string> list; };
struct StreamLabel { size_t port, at; std::string id; };

static void apply(WaveTrigger &b, const std::string &name, const std::string &kind, size_t u, double d, const std::string &s, const std::vector<std::string> &l)
{
    if (name == "setNumPoints") b.setNumPoints(u);
    else if (name == "setNumWindows") b.setNumWindows(u);
    else if (name == "setEventRate") b.setEventRate(d);
    else if (name == "setAlignment") b.setAlignment(u != 0);
    else if (name == "setSource") b.setSource(u);
    else if (name == "setHoldOff") b.setHoldOff(u);
    else if (name == "setSlope") b.setSlope(s);
    else if (name == "setMode") b.setMode(s);
    else if (name == "setLevel") b.setLevel(d);
    else if (name == "setPosition") b.setPosition(u);
    else if (name == "setLabelId") b.setLabelId(s);
    else if (name == "setIdsList") b.setIdsList(l);
    else { std::fprintf(stderr, "unknown setter %s\n", name.c_str()); std::exit(4); }
    (void)kind;
}
static void readValue(std::istream &c, std::string &kind, size_t &u, double &d, std::string &s, std::vector<std::string> &l)
{
    c >> kind;
    u = 0; d = 0; s.clear(); l.clear();
    if (kind == "u") c >> u;
    else if (kind == "d") c >> d;
    else if (kind == "s") { c >> s; if (s == "-") s.clear(); }
    else { size_t n; c >> n; l.resize(n); for (auto &x : l) c >> x; }
}
static unsigned long long bitsOf(double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream c(argv[1]);
    size_t nports;
    c >> nports;
    std::vector<std::string> dtypes(nports);
    std::vector<std::vector<char>> streams(nports);
    std::vector<size_t> total(nports), es(nports);
    for (size_t p = 0; p < nports; p++) {
        std::string file;
        c >> dtypes[p] >> total[p] >> file;
        std::ifstream in(file, std::ios::binary);
        streams[p].assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        es[p] = Pothos::DType(dtypes[p]).size();
        if (streams[p].size() != total[p] * es[p]) return 5;
    }
    WaveTrigger b;
    b.setNumPorts(nports);
    size_t nset;
    c >> nset;
    for (size_t i = 0; i < nset; i++) {
        std::string name, kind, s; size_t u; double d; std::vector<std::string> l;
        c >> name;
        readValue(c, kind, u, d, s, l);
        apply(b, name, kind, u, d, s, l);
    }
    size_t nlab;
    c >> nlab;
    std::vector<StreamLabel> slabels(nlab);
    for (auto &l : slabels) c >> l.port >> l.at >> l.id;
    size_t nfeed;
    c >> nfeed;
    std::vector<size_t> feed(nfeed);
    for (auto &f : feed) c >> f;
    size_t nev, lastEvent = 0;
    c >> nev;
    std::vector<Event> events(nev);
    for (auto &e : events) {
        c >> e.call >> e.type;
        if (e.type == "set") { c >> e.name; readValue(c, e.kind, e.u, e.d, e.sval, e.list); }
        else if (e.type == "plant") { c >> e.port >> e.sval; }
        else if (e.type == "packet") { c >> e.port >> e.sval >> e.u; }
        else { c >> e.port >> e.name >> e.u; }
        if (e.sval == "-") e.sval.clear();
        lastEvent = std::max(lastEvent, e.call + 1);
    }
    b.activate();
    std::vector<std::string> planted = dtypes;
    std::vector<size_t> pos(nports, 0);
    for (size_t k = 0; k < MAX_CALLS; k++) {
        for (const auto &e : events) {
            if (e.call != k) continue;
            if (e.type == "set") apply(b, e.name, e.kind, e.u, e.d, e.sval, e.list);
            else if (e.type == "plant") planted[e.port] = e.sval;
            else if (e.type == "packet") {
                Pothos::Packet pkt;
                const Pothos::DType dt = e.sval.empty() ? Pothos::DType() : Pothos::DType(e.sval);
                pkt.payload = Pothos::BufferChunk(dt, e.u / dt.size());
                for (size_t i = 0; i < e.u; i++) pkt.payload.as<unsigned char *>()[i] = (unsigned char)(i + 1);
                pkt.labels.push_back(Pothos::Label("m", Pothos::Object(), 1, 1));
                b.input(e.port)->msgs.push_back(Pothos::Object(pkt));
            } else {
                b.input(e.port)->msgs.push_back(Pothos::Object(Pothos::Label(e.name, Pothos::Object(), e.u, 1)));
            }
        }
        const size_t f = feed[std::min(k, nfeed - 1)];
        bool offeredAll = true;
        for (size_t p = 0; p < nports; p++) {
            auto port = b.input(p);
            const size_t m = std::min(f, total[p] - pos[p]);
            offeredAll = offeredAll and m == total[p] - pos[p];
            port->buf = Pothos::BufferChunk::view(streams[p].data() + pos[p] * es[p], m * es[p], planted[p].empty() ? Pothos::DType() : Pothos::DType(planted[p]));
            port->labs.clear();
            for (const auto &l : slabels)
                if (l.port == p and l.at >= pos[p] and l.at < pos[p] + m) port->labs.push_back(Pothos::Label(l.id, Pothos::Object(), (l.at - pos[p]) * es[p], es[p]));
            port->consumed = 0; port->reserve = 0; port->reserveSet = false;
        }
        b.out.posted.clear();
        b.yielded = false;
        b.work();
        std::printf("call\n");
        bool any = false;
        for (size_t p = 0; p < nports; p++) {
            auto port = b.input(p);
            std::printf("port %zu %lld\n", port->consumed, port->reserveSet ? (long long)port->reserve : -1LL);
            any = any or port->consumed != 0;
            std::vector<Pothos::Label> inside;
            for (const auto &l : port->labs) if (l.index < port->consumed) inside.push_back(l);
            port->labs.swap(inside);
            if (not port->labs.empty()) b.propagateLabels(port);
            if (port->consumed % es[p]) return 6;
            pos[p] += port->consumed / es[p];
        }
        std::printf("yield %d\n", b.yielded ? 1 : 0);
        for (const auto &m : b.out.posted) {
            if (m.type() == typeid(Pothos::Packet)) {
                const auto &pkt = m.extract<Pothos::Packet>();
                const auto ix = pkt.metadata.find("index"), ps = pkt.metadata.find("position"), lv = pkt.metadata.find("level");
                std::printf("msg packet %d %d %d %llu %d %llu %s %zu %zu\n", ix != pkt.metadata.end(), ix != pkt.metadata.end() ? ix->second.extract<int>() : 0,
                            ps != pkt.metadata.end(), ps != pkt.metadata.end() ? bitsOf(ps->second.extract<double>()) : 0ULL, lv != pkt.metadata.end(),
                            lv != pkt.metadata.end() ? bitsOf(lv->second.extract<double>()) : 0ULL, pkt.payload.dtype ? pkt.payload.dtype.name().c_str() : "-",
                            pkt.payload.length, pkt.labels.size());
                for (const auto &l : pkt.labels) std::printf("plabel %s %llu %zu\n", l.id.c_str(), l.index, l.width);
                std::printf("payload -");
                for (size_t i = 0; i < pkt.payload.length; i++) std::printf("%02x", pkt.payload.as<const unsigned char *>()[i]);
                std::printf("\n");
            } else if (m.type() == typeid(Pothos::Label)) {
                const auto &l = m.extract<Pothos::Label>();
                std::printf("msg label %s %llu %zu\n", l.id.c_str(), l.index, l.width);
            } else {
                std::printf("msg other\n");
            }
        }
        if (offeredAll and not any and b.out.posted.empty() and not b.yielded and k + 1 > lastEvent - (lastEvent ? 1 : 0)) return 0;
    }
    return 3;
}
"""

FLAGS = ["-std=c++11", "-O3", "-ffp-contract=off", "-fno-fast-math", "-w"]


def value_words(v):
    if isinstance(v, bool):
        return ["u", int(v)]
    if isinstance(v, int):
        return ["u", v]
    if isinstance(v, float):
        return ["d", repr(v)]
    if isinstance(v, str):
        return ["s", v or "-"]
    return ["l", len(v)] + list(v)


def reference_calls(exe, tmp, case, streams):
    words = [len(case.dtypes)]
    for p, dt in enumerate(case.dtypes):
        f = os.path.join(tmp, "x%d.bin" % p)
        np.ascontiguousarray(streams[p]).tofile(f)
        words += [dt, len(streams[p]), f]
    words.append(len(case.settings))
    for name, v in case.settings:
        words += [name] + value_words(v)
    labs = [(p, at, lid) for p, ls in sorted(case.labels.items()) for at, lid in ls]
    words.append(len(labs))
    for l in labs:
        words += list(l)
    words += [len(case.feed)] + list(case.feed)
    evs = [(k, ev) for k, es in sorted(case.events.items()) for ev in es]
    words.append(len(evs))
    for k, ev in evs:
        if ev[0] == "set":
            words += [k, "set", ev[1]] + value_words(ev[2])
        elif ev[0] == "plant":
            words += [k, "plant", ev[1], ev[2] or "-"]
        elif ev[0] == "packet":
            words += [k, "packet", ev[1], ev[2] or "-", ev[3]]
        else:
            words += [k, "label", ev[1], ev[2], ev[3]]
    cfg = os.path.join(tmp, "cfg.txt")
    open(cfg, "w").write(" ".join(str(w) for w in words) + "\n")
    lines = subprocess.check_output([exe, cfg]).decode().splitlines()
    calls = []
    for ln in lines:
        w = ln.split()
        if w[0] == "call":
            calls.append(([], [], False, []))
        elif w[0] == "port":
            calls[-1][0].append(int(w[1]))
            calls[-1][1].append(int(w[2]))
        elif w[0] == "yield":
            calls[-1] = calls[-1][:2] + (w[1] == "1", calls[-1][3])
        elif w[0] == "msg" and w[1] == "packet":
            calls[-1][3].append(["packet", int(w[3]) if w[2] == "1" else None, int(w[5]) if w[4] == "1" else None, int(w[7]) if w[6] == "1" else None,
                                 None if w[8] == "-" else w[8], b"", []])
        elif w[0] == "plabel":
            calls[-1][3][-1][6].append((w[1], int(w[2]), int(w[3])))
        elif w[0] == "payload":
            calls[-1][3][-1][5] = bytes.fromhex(w[1][1:])
        elif w[0] == "msg" and w[1] == "label":
            calls[-1][3].append(("label", w[2], int(w[3]), int(w[4])))
        else:
            calls[-1][3].append(("other",))
    return [(c, r, y, [tuple(m) for m in ms]) for c, r, y, ms in calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "trigger.npz"))
    args = ap.parse_args()
    data = dict(names=np.array([c.name for c in M.CASES]))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER.replace("MAX_CALLS", str(M.MAX_CALLS)))
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "standin_trigger"), "-I" + args.reference, src, "-o", exe])
        for k, case in enumerate(M.CASES):
            streams = [M.make_stream(case, p) for p in range(len(case.dtypes))]
            ref = reference_calls(exe, tmp, case, streams)
            model = M.flatten(M.model_calls(case, streams))
            assert len(ref) == len(model), (case.name, len(ref), len(model))
            for j, (r, m) in enumerate(zip(ref, model)):
                assert r == m, (case.name, j, r, m)
            payload, calls = b"", []
            for consumed, reserve, yielded, msgs in ref:
                ms = []
                for m in msgs:
                    if m[0] == "packet":
                        ms.append(["packet", m[1], m[2], m[3], m[4], len(payload), len(m[5]), [list(l) for l in m[6]]])
                        payload += m[5]
                    else:
                        ms.append(list(m))
                calls.append([consumed, reserve, yielded, ms])
            for p, x in enumerate(streams):
                data["x%d_%d" % (k, p)] = x
            data["calls%d" % k] = np.array(json.dumps(calls))
            data["payload%d" % k] = np.frombuffer(payload, np.uint8)
            npk = sum(1 for c in ref for m in c[3] if m[0] == "packet")
            print("%-30s %3d calls, %3d packets, %2d labels, %6d payload bytes" % (case.name, len(ref), npk, sum(1 for c in ref for m in c[3] if m[0] == "label"),
                                                                                  len(payload)))
    np.savez_compressed(args.out, **data)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
