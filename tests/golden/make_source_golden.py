"""Writes tests/golden/source.npz: what /comms/waveform_source and /comms/noise_source of the reference produce.

Run where a C++ compiler and the reference tree are.  A driver of this project's own (DRIVER below) is written into a temporary directory
together with a stand-in Pothos/Framework.hpp of this project's own (FRAMEWORK: Block with one output port, registerCall as a no-op,
isActive, the registry and the exception types).  The driver includes waveform/WaveformSource.cpp resp. waveform/NoiseSource.cpp BY PATH
from the reference tree and is compiled with the oracle's flags.  For the noise source std::random_device is replaced, by a macro in
front of the include, with a stand-in that returns a fixed seed.  Nothing compiled and no text of the reference is kept: the file holds
parameters and recorded outputs only.  No test reads the reference tree.

Cases (tests/source_model.py):
  matrix/<type>/<wave>     12 types x CONST, SINE, RAMP, SQUARE at freq 0.1, rate 1; amplitude 100 and offset (25, -50) for the integer
                           types, 1 and (0.25, -0.5) otherwise; work() calls of 257, 300 and 43 elements
  neg, zero, slow, slowest, res, retune / <type>   on complex_float32, complex_int16, float64: freq -0.25 (step = 3072 mod 4096, period
                           4), freq 0 (period 1), freq 1e-4 (262144 entries, step 26; 600 outputs), freq 1e-6 (2^20 entries, step 1; 600
                           outputs), res 1e-3 with freq 0.1 (16384 entries, step 1638), freq 0.1 for 300 elements and then freq 1e-4 for
                           300 more (the carried index enters the larger table)
  unachievable             freq 1e-7: the reference's exception text
  noise/<type>/<wave>      UNIFORM, NORMAL, LAPLACE, POISSON with seed 20261018, mean 0.5, b 0.25 on complex_float64, float32 and
                           complex_int16 (amplitude 100): the 4096-entry table and five work() calls of 100 elements
Per case: out/<case> (the calls one after another), state/<case> (entries, step, mask and index after every op, as uint64 rows) and
sha/<case> (the SHA-256 of the table after the LAST op).  The table itself, table/<case>, is kept where the file's size allows it: the
matrix on the three further types, and every noise table but complex_float64's (4 x 64 KiB of random doubles do not compress; their
windows and their hash are kept).  noise_imag_first records the order in which the compiled reference draws the two components of an
entry: the C++ it is written in leaves that order to the compiler.

    python tests/golden/make_source_golden.py [--reference /root/reference] [--out tests/golden/source.npz]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import source_model as M  # noqa: E402

FRAMEWORK = r"""
// stand-in for Pothos/Framework.hpp: what the two sources of waveform/ use, and no more
#pragma once
#include <complex>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <vector>
#define POTHOS_FCN_TUPLE(c, m) #m, &c::m
namespace Pothos {
struct Exception : std::runtime_error {
    Exception(const std::string &where, const std::string &what) : std::runtime_error(what), where(where) {}
    std::string where;
};
struct InvalidArgumentException : Exception { using Exception::Exception; };
struct DType {
    DType() : t(&typeid(void)) {}
    DType(const std::type_info &ti) : t(&ti) {}
    bool operator==(const DType &o) const { return *t == *o.t; }
    std::string toString() const { return t->name(); }
    const std::type_info *t;
};
struct Buffer {
    void *p;
    template <typename T> operator T *() const { return static_cast<T *>(p); }
};
struct OutputPort {
    Buffer buffer() const { return Buffer{mem}; }
    size_t elements() const { return room; }
    void produce(size_t n) { produced += n; }
    void *mem = nullptr;
    size_t room = 0, produced = 0;
};
class Block {
public:
    virtual ~Block() {}
    virtual void activate() {}
    virtual void work() {}
    void setupOutput(size_t, const DType &) {}
    template <typename... A> void registerCall(A &&...) {}
    bool isActive() const { return active; }
    OutputPort *output(size_t) { return &port; }
    bool active = false;
    OutputPort port;
};
struct BlockRegistry {
    template <typename F> BlockRegistry(const std::string &, F) {}
};
}  // namespace Pothos
"""

DRIVER = r"""
// driver <type> <out.bin> <table.bin> op...   (ops: wave W | rate x | freq x | res x | ampl re im | offset re im | mean x | b x |
// activate | work n); prints one "state entries step mask index" line per op, "throw where|what" for an exception, and for the noise
// source "order real_first|imag_first"
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <random>
#include <string>
#include <vector>
#include <Pothos/Framework.hpp>
#define private public
#ifdef PCX_NOISE
namespace std { struct pcx_fixed_seed_device { unsigned operator()() { return PCX_SEED; } }; }
#define random_device pcx_fixed_seed_device
#include "waveform/NoiseSource.cpp"
#undef random_device
template <typename T> using Source = NoiseSource<T>;
#else
#include "waveform/WaveformSource.cpp"
template <typename T> using Source = WaveformSource<T>;
#endif
#undef private

template <typename T>
int run(int argc, char **a)
{
    Source<T> blk;
    FILE *out = std::fopen(a[2], "wb");
    if (!out) return 2;
    try {
        for (int i = 4; i < argc; i++) {
            const std::string op = a[i];
            if (op == "wave") blk.setWaveform(a[++i]);
            else if (op == "ampl") { const double re = std::atof(a[++i]), im = std::atof(a[++i]); blk.setAmplitude(std::complex<double>(re, im)); }
            else if (op == "offset") { const double re = std::atof(a[++i]), im = std::atof(a[++i]); blk.setOffset(std::complex<double>(re, im)); }
#ifdef PCX_NOISE
            else if (op == "mean") blk.setMean(std::atof(a[++i]));
            else if (op == "b") blk.setB(std::atof(a[++i]));
#else
            else if (op == "rate") blk.setSampleRate(std::atof(a[++i]));
            else if (op == "freq") blk.setFrequency(std::atof(a[++i]));
            else if (op == "res") blk.setResolution(std::atof(a[++i]));
#endif
            else if (op == "activate") { blk.active = true; blk.activate(); }
            else if (op == "work") {
                const size_t n = std::strtoull(a[++i], 0, 10);
                std::vector<T> buf(n);
                blk.port.mem = buf.data();
                blk.port.room = n;
                blk.port.produced = 0;
                blk.work();
                if (blk.port.produced != n) return 4;
                if (std::fwrite(buf.data(), sizeof(T), n, out) != n) return 3;
            } else return 1;
#ifdef PCX_NOISE
            std::printf("state %zu 1 4095 %zu\n", blk._table.size(), blk._index);
#else
            std::printf("state %zu %zu %zu %zu\n", blk._table.size(), blk._step, blk._mask, blk._index);
#endif
        }
    } catch (const Pothos::Exception &e) {
        std::printf("throw %s|%s\n", e.where.c_str(), e.what());
    }
    std::fclose(out);
    FILE *tab = std::fopen(a[3], "wb");
    if (!tab || std::fwrite(blk._table.data(), sizeof(T), blk._table.size(), tab) != blk._table.size()) return 3;
    std::fclose(tab);
    return 0;
}

int main(int argc, char **a)
{
    if (argc < 4) return 1;
#ifdef PCX_NOISE
    {   // which component of an entry is drawn first: UNIFORM at amplitude 1 and offset 0 against the generator's first two draws
        NoiseSource<std::complex<double>> probe;
        probe.setWaveform("UNIFORM");
        probe.active = true;
        probe.activate();
        std::mt19937 g(PCX_SEED);
        std::uniform_real_distribution<> u(-1.0, 1.0);
        const double first = u(g), second = u(g);
        if (probe._table[0] == std::complex<double>(first, second)) std::printf("order real_first\n");
        else if (probe._table[0] == std::complex<double>(second, first)) std::printf("order imag_first\n");
        else return 5;
    }
#endif
    const std::string t = a[1];
#define PCX_T(name, type) if (t == name) return run<type>(argc, a); if (t == "complex_" name) return run<std::complex<type>>(argc, a);
    PCX_T("float64", double) PCX_T("float32", float) PCX_T("int64", int64_t) PCX_T("int32", int32_t) PCX_T("int16", int16_t) PCX_T("int8", int8_t)
    return 1;
}
"""

# the oracle's flags (oracle/Makefile)
FLAGS = ["-std=c++11", "-O3", "-ffp-contract=off", "-fno-fast-math", "-w"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCX_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(HERE, "source.npz"))
    args = ap.parse_args()
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Pothos"))
        open(os.path.join(tmp, "Pothos", "Framework.hpp"), "w").write(FRAMEWORK)
        src = os.path.join(tmp, "driver.cpp")
        open(src, "w").write(DRIVER)
        wave_exe, noise_exe = os.path.join(tmp, "wave"), os.path.join(tmp, "noise")
        inc = ["-I" + tmp, "-I" + args.reference]
        subprocess.check_call(["g++"] + FLAGS + inc + [src, "-o", wave_exe])
        subprocess.check_call(["g++"] + FLAGS + inc + ["-DPCX_NOISE", "-DPCX_SEED=%du" % M.NOISE_SEED, src, "-o", noise_exe])

        def run(exe, dtype, ops):
            fout, ftab = os.path.join(tmp, "out.bin"), os.path.join(tmp, "table.bin")
            text = subprocess.check_output([exe, dtype, fout, ftab] + [str(o) for o in ops]).decode()
            lines = text.splitlines()
            states = np.array([[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("state ")], dtype=np.uint64).reshape(-1, 4)
            thrown = [ln[6:] for ln in lines if ln.startswith("throw ")]
            order = [ln[6:] for ln in lines if ln.startswith("order ")]
            sc = M.np_scalar(dtype)
            out = np.fromfile(fout, dtype=sc).reshape(M.shape(dtype, -1))
            tab = np.fromfile(ftab, dtype=sc).reshape(M.shape(dtype, -1))
            return out, tab, states, thrown, order

        for name, dt, wave, ops in M.waveform_cases():
            ampl, offset = M.ampl_offset(dt)
            argv = ["wave", wave, "rate", 1.0, "ampl", ampl[0], ampl[1], "offset", offset[0], offset[1], "activate"]
            for op, v in ops:
                argv += [op, repr(v) if op != "work" else v]
            out, tab, states, thrown, _ = run(wave_exe, dt, argv)
            assert not thrown, (name, thrown)
            data["out/" + name], data["state/" + name], data["sha/" + name] = out, states, np.array(M.digest(tab))
            if name.startswith("matrix/") and dt in M.FURTHER_TYPES:
                data["table/" + name] = tab
        _, _, _, thrown, _ = run(wave_exe, "complex_float32", ["wave", "SINE", "activate", "freq", repr(1e-7)])
        assert len(thrown) == 1
        data["unachievable"] = np.array(thrown[0])
        _, _, _, thrown, _ = run(wave_exe, "complex_float32", ["activate", "wave", "TRIANGLE"])
        assert len(thrown) == 1
        data["unknown_wave"] = np.array(thrown[0])
        for name, dt, wave in M.noise_cases():
            k = 100.0 if M.is_integer(dt) else 1.0
            argv = ["wave", wave, "mean", M.NOISE_MEAN, "b", M.NOISE_B, "ampl", k, 0.0, "offset", 0.0, 0.0, "activate"]
            for n in M.NOISE_CALLS:
                argv += ["work", n]
            out, tab, states, thrown, order = run(noise_exe, dt, argv)
            assert not thrown and len(order) == 1, (name, thrown, order)
            data["out/" + name], data["state/" + name], data["sha/" + name] = out, states, np.array(M.digest(tab))
            if dt != "complex_float64":
                data["table/" + name] = tab
            data["noise_imag_first"] = np.array(order[0] == "imag_first")
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes; noise draws %s" % (args.out, len(data), os.path.getsize(args.out), "imag first" if data["noise_imag_first"] else "real first"))


if __name__ == "__main__":
    main()
