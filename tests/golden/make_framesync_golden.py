"""Writes tests/golden/framesync.npz: what /comms/frame_sync of the reference does, call by call, on the streams of
tests/framesync_model.py's CASES.

Run where a C++ compiler and the reference tree are.  A driver of this project's own (DRIVER below) is written into a temporary
directory.  It includes digital/FrameSync.cpp (and through it digital/FrameHelper.hpp) BY PATH from the reference tree, is compiled with
the oracle's flags against the stand-in header tests/golden/standin_sync/Pothos/Framework.hpp, and runs the block's own work().  Nothing
compiled is kept and no text of the reference is kept: the file holds parameters and recorded outputs only.  No test reads the reference
tree.

The driver keeps the whole stream in one array behind corrDurThresh + 2 zeros, so that the reference's read in front of a call's buffer
(the frame offset lies up to corrDurThresh elements in front of it) stays inside the array and sees what the port's history would
hold.  It hands out base + consumed and loops work() under the case's FEED SCHEDULE -- call k sees feed[min(k, len - 1)] elements past
the consumed ones, or what is left -- with an output buffer of the case's capacity (the call's input length where the case names none),
until a call that sees the whole rest consumes and produces nothing.

Per case the file holds: the stream (in the case's own type, as `tuned` chose it), and for BOTH instantiations of the
reference (complex<float> on the stream rounded to float32, complex<double> on the stream as it is) per call consumed, produced, the
reserve and the labels (`calls`, `labels` of the case's own type; `other_calls`, `other_labels` of the other one); of the instantiation of
the case's own type also the produced elements, the values of the phase labels and the
estimates at the maximum (the block's private members, read through the driver) after every call.  The maker asserts the condition of
the parity contract on every stream (the model's margins) and that the two instantiations and the model agree on every integer.

    python tests/golden/make_framesync_golden.py [--reference /root/reference] [--out tests/golden/framesync.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import framesync_model as M  # noqa: E402

DRIVER = r"""
// driver <f|d> <cfg.txt> <stream.bin> <out.bin>: the calls of one case; prints per call
//   "call <consumed> <produced> <reserve> <labels> <scale> <deltaFc> <phaseOff>" and per label "label <id> <index> <width> <is double> <value>"
#include <algorithm>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include <Pothos/Framework.hpp>
#define private public
#include "digital/FrameSync.cpp"
#undef private

template <typename R>
static int run(const char *cfg, const char *fin, const char *fout)
{
    typedef std::complex<R> E;
    std::ifstream c(cfg);
    size_t sw, dw, P;
    c >> sw >> dw >> P;
    std::vector<E> pre(P);
    for (size_t i = 0; i < P; i++) { double re, im; c >> re >> im; pre[i] = E(R(re), R(im)); }
    unsigned id; std::string mode, sid, eid, pid; double thresh; long cap; size_t nfeed;
    c >> id >> mode >> thresh >> sid >> eid >> pid >> cap >> nfeed;
    std::vector<size_t> feed(nfeed);
    for (size_t i = 0; i < nfeed; i++) c >> feed[i];
    auto name = [](const std::string &s) { return s == "-" ? std::string() : s; };
    FrameSync<E> b;
    b.setSymbolWidth(sw);
    b.setDataWidth(dw);
    b.setPreamble(pre);
    b.setHeaderId((unsigned char)id);
    b.setOutputMode(mode);
    b.setInputThreshold(R(thresh));
    b.setFrameStartId(name(sid));
    b.setFrameEndId(name(eid));
    b.setPhaseOffsetID(name(pid));
    std::ifstream in(fin, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const size_t total = raw.size() / sizeof(E), pad = b._corrDurThresh + 2;
    std::vector<E> x(pad + total, E(0));
    std::memcpy(x.data() + pad, raw.data(), total * sizeof(E));
    std::ofstream out(fout, std::ios::binary);
    b.activate();
    b._deltaFcMax = b._phaseOffMax = b._scaleAtMax = 0;
    size_t pos = 0;
    for (size_t k = 0; k < 100000; k++) {
        const size_t n_in = std::min(feed[std::min(k, nfeed - 1)], total - pos), room = cap < 0 ? n_in : size_t(cap);
        std::vector<E> y(room + 1, E(0));
        b.give(x.data() + pad + pos, n_in, y.data(), room);
        b.work();
        std::printf("call %zu %zu %zu %zu %.17g %.17g %.17g\n", b.in.consumed, b.out.produced, b.in.reserve, b.out.posted.size(), double(b._scaleAtMax),
                    double(b._deltaFcMax), double(b._phaseOffMax));
        for (const auto &l : b.out.posted)
            std::printf("label %s %llu %zu %d %.17g\n", l.id.c_str(), l.index, l.width, l.data.is_double ? 1 : 0, l.data.is_double ? l.data.real : double(l.data.number));
        out.write(reinterpret_cast<const char *>(y.data()), b.out.produced * sizeof(E));
        pos += b.in.consumed;
        if (b.in.consumed == 0 and b.out.produced == 0 and n_in == total - pos) return 0;
    }
    return 3;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    return argv[1][0] == 'f' ? run<float>(argv[2], argv[3], argv[4]) : run<double>(argv[2], argv[3], argv[4]);
}
"""

FLAGS = ["-std=c++11", "-O3", "-ffp-contract=off", "-fno-fast-math", "-w"]
IDS = {"frame_start": "s", "frame_end": "e", "phase_offset": "p"}


def reference_calls(exe, tmp, case, x, flavour):
    """the calls of one instantiation ('f' or 'd') on the stream x -> [Call] with state (scale, delta_fc, phase_off)"""
    s = case.settings
    ct = np.complex64 if flavour == "f" else np.complex128
    fcfg, fin, fout = (os.path.join(tmp, n) for n in ("cfg.txt", "in.bin", "out.bin"))
    ids = [IDS[k] if v else "-" for k, v in (("frame_start", s.start_id), ("frame_end", s.end_id), ("phase_offset", s.phase_id))]
    words = [s.sw, s.dw, len(s.preamble)] + [repr(float(v)) for p in s.preamble for v in (p.real, p.imag)]
    words += [s.header_id, s.mode, repr(float(s.thresh))] + ids + [-1 if case.out_cap is None else case.out_cap, len(case.feed)] + list(case.feed)
    open(fcfg, "w").write(" ".join(str(w) for w in words) + "\n")
    x.astype(ct).tofile(fin)
    lines = subprocess.check_output([exe, flavour, fcfg, fin, fout]).decode().splitlines()
    produced = np.fromfile(fout, ct)
    kinds = {v: k for k, v in IDS.items()}
    calls, at = [], 0
    for ln in lines:
        w = ln.split()
        if w[0] == "call":
            n = int(w[2])
            calls.append(M.Call(int(w[1]), n, int(w[3]), [], produced[at:at + n], dict(scale=float(w[5]), delta_fc=float(w[6]), phase_off=float(w[7]))))
            at += n
        else:
            calls[-1].labels.append((kinds[w[1]], int(w[2]), int(w[3]), float(w[5]) if w[4] == "1" else int(float(w[5]))))
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "framesync.npz"))
    args = ap.parse_args()
    M.GOLDEN_PATH = None                    # the streams are chosen afresh, not read back
    data = dict(names=np.array([c.name for c in M.CASES]))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++"] + FLAGS + ["-I" + os.path.join(HERE, "standin_sync"), "-I" + args.reference, src, "-o", exe])
        for k, case in enumerate(M.CASES):
            own = "f" if case.dtype == "complex_float32" else "d"
            for seed_from in range(0, 480, 48):         # a stream on which the reference itself disagrees with the model is not recorded: the next seeds
                _, s, x, mt, ct, co, margins, _, _ = M.prepare(case, seeds=range(seed_from, seed_from + 48))
                ref = {f: reference_calls(exe, tmp, case, x, f) for f in "fd"}
                if M.integers(ref["f"]) == M.integers(ref["d"]) == M.integers(ct):
                    break
            else:
                raise AssertionError("%s: the reference and the model disagree on every stream tried" % case.name)
            assert M.condition(mt.margins)[0], (case.name, margins)
            r = ref[own]
            o = ref["d" if own == "f" else "f"]
            data["other_calls%d" % k] = np.array([[c.consumed, c.produced, c.reserve, len(c.labels)] for c in o], np.int64)
            data["other_labels%d" % k] = np.array([[M.LABEL_KINDS.index(l[0]), l[1], l[2], 0 if l[0] == "phase_offset" else l[3]] for c in o for l in c.labels],
                                                  np.int64).reshape(-1, 4)
            data["x%d" % k] = x
            data["calls%d" % k] = np.array([[c.consumed, c.produced, c.reserve, len(c.labels)] for c in r], np.int64)
            data["labels%d" % k] = np.array([[M.LABEL_KINDS.index(l[0]), l[1], l[2], 0 if l[0] == "phase_offset" else l[3]] for c in r for l in c.labels],
                                            np.int64).reshape(-1, 4)
            data["phases%d" % k] = np.array([l[3] for c in r for l in c.labels if l[0] == "phase_offset"], np.float64)
            data["est%d" % k] = np.array([[c.state["scale"], c.state["delta_fc"], c.state["phase_off"]] for c in r], np.float64)
            data["out%d" % k] = np.concatenate([c.out for c in r]) if r else x[:0]
            print("%-28s %5d elements, %2d calls, margins %.3f %.3f %.3f" % ((case.name, len(x), len(r)) + tuple(min(m, 9.999) for m in margins)))
    np.savez_compressed(args.out, **data)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
