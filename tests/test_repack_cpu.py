"""CPU suite of /comms/bits_to_symbols, /comms/symbols_to_bits, /comms/bytes_to_symbols and /comms/symbols_to_bytes: the model
(tests/repack_model.py) against the recorded reference outputs (tests/golden/repack.npz) and against itself, the kernels' word
arithmetic (csrc/repack_core.hpp, compiled for the host) against the same recordings, the C ABI's argument checks, the registry of
libpcx_repack_blocks.so, the four descriptions and the blocks' defaults.  No device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import repack_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pothoscomms_amd", "csrc")
SRC = os.path.join(CSRC, "blocks", "repack_blocks.cpp")
REF = "/root/reference"
PATHS = sorted(p + n for p in ("/blocks/", "/comms/") for n in M.KINDS)
REF_FILES = {"bits_to_symbols": "BitsToSymbols.cpp", "symbols_to_bits": "SymbolsToBits.cpp", "bytes_to_symbols": "BytesToSymbols.cpp",
             "symbols_to_bytes": "SymbolsToBytes.cpp"}
COMMON_CALLS = {"setDevice": 1, "getDevice": 0, "setPortSlabBytes": 1, "getPortSlabBytes": 0}
OWN_CALLS = {"setModulus": 1, "getModulus": 0, "setBitOrder": 1, "getBitOrder": 0}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "repack.npz"))


def split(name):
    kind, order, w = name.split("/")
    return kind, order, int(w)


# ---- the model and the recording
def test_model_equals_every_recorded_case(golden):
    assert [str(k) for k in golden["cases"]] == M.CASES and len(M.CASES) == 64
    for name in M.CASES:
        kind, order, w = split(name)
        assert np.array_equal(M.convert(kind, golden["in_full"], w, order), golden["out/" + name]), name
        if kind in ("bits_to_symbols", "symbols_to_bits"):
            assert np.array_equal(M.convert(kind, golden["in_bits"], w, order), golden["out_bits/" + name]), name
        if kind == "symbols_to_bytes":
            masked = golden["in_full"] & np.uint8((1 << w) - 1)
            assert np.array_equal(M.convert(kind, masked, w, order), golden["out_masked/" + name]), name


def test_recording_covers_what_it_is_meant_to(golden):
    cases = [str(k) for k in golden["cases"]]
    assert len(cases) == 64 and len(set(cases)) == 64
    assert {split(c) for c in cases} == {(k, o, w) for k in M.KINDS for o in M.ORDERS for w in M.WIDTHS}
    x, b = golden["in_full"], golden["in_bits"]
    assert x.size == 1680 and b.size == 1680 and all(x.size % M.group(k, w)[0] == 0 for k in M.KINDS for w in M.WIDTHS)
    assert (x > 127).any() and len(np.unique(x)) > 250 and set(np.unique(b)) == {0, 1}
    assert ((x != 0) & (x & 1 == 0)).any()              # bits_to_symbols: non-zero is not "low bit set"
    for order in M.ORDERS:
        for w in M.WIDTHS:
            name = M.case_name("symbols_to_bytes", order, w)
            differ = int((golden["out/" + name] != golden["out_masked/" + name]).sum())
            assert (differ > 0) == (w < 8), (name, differ)
            assert golden["out/" + M.case_name("bytes_to_symbols", order, w)].max() < 1 << w
            assert golden["out/" + M.case_name("symbols_to_bits", order, w)].max() == 1
        # counting the low bit instead of testing for non-zero would give another answer
        name = M.case_name("bits_to_symbols", order, 3)
        assert not np.array_equal(M.bits_to_symbols(x & 1, 3, order), golden["out/" + name])


def test_the_two_probes_of_the_unmasked_pack():
    s = np.zeros(8, np.uint8)
    s[2] = 0xFF
    assert M.symbols_to_bytes(s, 3, "MSBit").tolist() == [0x7F, 0x80, 0x00]
    s[:] = 0
    s[3] = 0xFF
    assert M.symbols_to_bytes(s, 3, "MSBit").tolist() == [0x00, 0xF0, 0x00]
    # a symbol never reaches a byte its field does not touch, and always shows whole in the bytes it does
    for order in M.ORDERS:
        for w in range(1, 8):
            for j in range(8):
                s[:] = 0
                s[j] = 0xFF
                clean = M.symbols_to_bytes(s & np.uint8((1 << w) - 1), w, order)
                leaky = M.symbols_to_bytes(s, w, order)
                assert ((leaky != 0) == (clean != 0)).all() and ((leaky & clean) == clean).all(), (order, w, j)


def test_round_trips_in_the_model_with_clean_inputs():
    rng = np.random.default_rng(3)
    for order in M.ORDERS:
        for w in M.WIDTHS:
            payload = rng.integers(0, 256, 840, dtype=np.uint8)
            syms = M.convert("bytes_to_symbols", payload, w, order)
            assert syms.size == 840 * 8 // w and syms.max() < 1 << w
            assert np.array_equal(M.convert("symbols_to_bytes", syms, w, order), payload), (order, w)
            syms = rng.integers(0, 1 << w, 500).astype(np.uint8)
            bits = M.convert("symbols_to_bits", syms, w, order)
            assert bits.size == 500 * w and bits.max() <= 1
            assert np.array_equal(M.convert("bits_to_symbols", bits, w, order), syms), (order, w)
            # bits that are any non-zero value count the same
            assert np.array_equal(M.convert("bits_to_symbols", bits * np.uint8(0x80), w, order), syms), (order, w)


def test_group_table_and_label_ratios():
    assert [M.group("bytes_to_symbols", w) for w in M.WIDTHS] == [(1, 8), (1, 4), (3, 8), (1, 2), (5, 8), (3, 4), (7, 8), (1, 1)]
    assert [M.group("symbols_to_bytes", w) for w in M.WIDTHS] == [(8, 1), (4, 1), (8, 3), (2, 1), (8, 5), (4, 3), (8, 7), (1, 1)]
    assert [M.group("bits_to_symbols", w) for w in M.WIDTHS] == [(w, 1) for w in M.WIDTHS]
    assert [M.group("symbols_to_bits", w) for w in M.WIDTHS] == [(1, w) for w in M.WIDTHS]
    assert [M.label_ratio(k, 3) for k in M.KINDS] == [(1, 3), (3, 1), (8, 3), (3, 8)]
    assert M.reserve("symbols_to_bits", 5) is None and M.reserve("bits_to_symbols", 5) == 5 and M.reserve("bytes_to_symbols", 6) == 3


# ---- the kernels' word arithmetic, compiled for the host
DRIVER = r"""
// driver <kind 0..3> <msb> <in.bin> <out.bin> <n_in>: whole tiles of 32 symbols through the lane functions of repack_core.hpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "repack_core.hpp"
using namespace pcx::repack;
template <int KIND, int W, bool MSB>
static void run(const std::vector<unsigned char> &in, std::vector<unsigned char> &out)
{
    constexpr bool to_syms = KIND == 0 || KIND == 2, bits = KIND == 0 || KIND == 1;
    const size_t nsym = to_syms ? (bits ? in.size() / W : in.size() * 8 / W) : in.size();
    std::vector<unsigned char> packed(nsym * W / 8);
    if (to_syms) {
        if (bits) {
            for (size_t u = 0; u < in.size() / 16; u++) {
                uint64_t a, b;
                std::memcpy(&a, &in[16 * u], 8);
                std::memcpy(&b, &in[16 * u + 8], 8);
                const uint32_t f = gather16<MSB>(a, b);
                packed[2 * u] = (unsigned char)f;
                packed[2 * u + 1] = (unsigned char)(f >> 8);
            }
        } else {
            packed = in;
        }
        out.resize(nsym);
        for (size_t i = 0; i < nsym; i += 32) {
            uint32_t p[W], s[8];
            std::memcpy(p, &packed[i * W / 8], 4 * W);
            extract32<W, MSB>(p, s);
            std::memcpy(&out[i], s, 32);
        }
        return;
    }
    for (size_t i = 0; i < nsym; i += 32) {
        uint32_t p[W], s[8];
        std::memcpy(s, &in[i], 32);
        pack32<W, MSB, bits>(s, p);
        std::memcpy(&packed[i * W / 8], p, 4 * W);
    }
    if (!bits) { out = packed; return; }
    out.resize(nsym * W);
    for (size_t u = 0; u < packed.size() / 2; u++) {
        uint32_t o[4];
        spread16<MSB>(packed[2 * u] | (packed[2 * u + 1] << 8), o);
        std::memcpy(&out[16 * u], o, 16);
    }
}
template <int KIND, int W>
static void order(bool msb, const std::vector<unsigned char> &in, std::vector<unsigned char> &out)
{
    if (msb) run<KIND, W, true>(in, out); else run<KIND, W, false>(in, out);
}
template <int KIND>
static void width(int w, bool msb, const std::vector<unsigned char> &in, std::vector<unsigned char> &out)
{
    switch (w) {
    case 1: order<KIND, 1>(msb, in, out); break; case 2: order<KIND, 2>(msb, in, out); break;
    case 3: order<KIND, 3>(msb, in, out); break; case 4: order<KIND, 4>(msb, in, out); break;
    case 5: order<KIND, 5>(msb, in, out); break; case 6: order<KIND, 6>(msb, in, out); break;
    case 7: order<KIND, 7>(msb, in, out); break; case 8: order<KIND, 8>(msb, in, out); break;
    }
}
int main(int argc, char **a)
{
    if (argc != 6) return 1;
    const size_t n = std::strtoull(a[5], 0, 10);
    std::vector<unsigned char> in(n), out;
    FILE *f = std::fopen(a[3], "rb");
    if (!f || std::fread(in.data(), 1, n, f) != n) return 2;
    std::fclose(f);
    f = std::fopen(a[4], "wb");
    for (int w = 1; w <= 8; w++) {
        switch (std::atoi(a[1])) {
        case 0: width<0>(w, std::atoi(a[2]) != 0, in, out); break;
        case 1: width<1>(w, std::atoi(a[2]) != 0, in, out); break;
        case 2: width<2>(w, std::atoi(a[2]) != 0, in, out); break;
        default: width<3>(w, std::atoi(a[2]) != 0, in, out);
        }
        if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 3;
    }
    std::fclose(f);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_kernel_word_arithmetic_equals_every_recorded_case(golden, tmp_path):
    """extract32 / pack32 / gather16 / spread16 are the whole arithmetic of repack.hip; a host compiler runs the same text.  The 1680
    inputs are repeated to 3360 x 8 = 26880 elements, a whole number of lanes (32 symbols) at every width."""
    src, exe = tmp_path / "driver.cpp", tmp_path / "driver"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I" + CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    for inputs, outs in (("in_full", "out/"), ("in_bits", "out_bits/")):
        x = np.tile(golden[inputs], 16)
        x.tofile(str(tmp_path / "in.bin"))
        for ki, kind in enumerate(M.KINDS):
            if inputs == "in_bits" and kind not in ("bits_to_symbols", "symbols_to_bits"):
                continue
            for order in M.ORDERS:
                subprocess.check_call([str(exe), str(ki), str(int(order == "MSBit")), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(x.size)])
                got = np.fromfile(str(tmp_path / "out.bin"), dtype=np.uint8)
                at = 0
                for w in M.WIDTHS:
                    m = M.out_elems(kind, w, x.size)
                    want = np.tile(golden[outs + M.case_name(kind, order, w)], 16)
                    assert np.array_equal(got[at:at + m], want), (kind, order, w)
                    at += m
                assert at == got.size


# ---- the C ABI (no device is touched)
def test_abi_argument_errors_come_before_any_device_call(pcx):
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    err = pcx._lib.last_error
    buf = (C.c_ubyte * 256)()
    base = C.addressof(buf)
    h, mod, msb = C.c_void_p(), C.c_uint(), C.c_int()
    a, b = C.c_size_t(), C.c_size_t()
    assert L.pcx_repack_create(0, None) == E
    for bad in (-1, 4, 99):
        assert L.pcx_repack_create(bad, C.byref(h)) == E and "unknown kind" in err()
    assert L.pcx_repack_set_modulus(None, 3) == E and "null handle" in err()
    assert L.pcx_repack_set_modulus(None, 0) == E and "null handle" in err()
    assert L.pcx_repack_get_modulus(None, C.byref(mod)) == E
    assert L.pcx_repack_set_bit_order(None, 1) == E and "null handle" in err()
    assert L.pcx_repack_get_bit_order(None, C.byref(msb)) == E
    assert L.pcx_repack_get_group(None, C.byref(a), C.byref(b)) == E
    assert L.pcx_repack_get_geometry(None, C.byref(a), C.byref(b)) == E
    assert L.pcx_repack_process(None, buf, buf, 8) == E and "null handle" in err()
    assert L.pcx_repack_process_dev(None, buf, buf, 8, None) == E and "null handle" in err()
    for ki, kind in enumerate(M.KINDS):
        assert L.pcx_repack_create(ki, C.byref(h)) == 0
        try:
            # the constructor's values
            assert L.pcx_repack_get_modulus(h, C.byref(mod)) == 0 and mod.value == 1
            assert L.pcx_repack_get_bit_order(h, C.byref(msb)) == 0 and msb.value == int(M.FRESH_ORDER[kind] == "MSBit")
            assert L.pcx_repack_set_modulus(h, 3) == 0
            for bad in (0, 9, 255, 256, 2 ** 32 - 1):
                assert L.pcx_repack_set_modulus(h, bad) == E and "Modulus must be between 1 and 8 inclusive" in err(), bad
                assert L.pcx_repack_get_modulus(h, C.byref(mod)) == 0 and mod.value == 3          # refused: kept
            assert L.pcx_repack_get_group(h, None, C.byref(b)) == E and L.pcx_repack_get_geometry(h, C.byref(a), None) == E
            assert L.pcx_repack_get_group(h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == M.group(kind, 3)
            gin, gout = M.group(kind, 3)
            # n == 0 comes before everything but the handle
            assert L.pcx_repack_process(h, None, None, 0) == 0 and L.pcx_repack_process_dev(h, None, None, 0, None) == 0
            # not a whole group comes before the buffers
            if gin > 1:
                for n in (1, gin - 1, gin + 1, 5 * gin + 1):
                    assert L.pcx_repack_process(h, None, None, n) == E and "not a whole group" in err(), (kind, n)
                    assert L.pcx_repack_process_dev(h, None, None, n, None) == E and "not a whole group" in err(), (kind, n)
            assert L.pcx_repack_process(h, None, buf, 4 * gin) == E and "null buffer" in err()
            assert L.pcx_repack_process(h, buf, None, 4 * gin) == E and "null buffer" in err()
            assert L.pcx_repack_process_dev(h, buf, None, 4 * gin, None) == E and "null buffer" in err()
            # overlap in both directions: 4 groups in at `base + i`, their outputs at `base + o`
            nin, nout = 4 * gin, 4 * gout
            for i, o in ((0, 0), (0, nin - 1), (nout - 1, 0), (1, 0), (0, 1)):
                assert L.pcx_repack_process_dev(h, C.c_void_p(base + i), C.c_void_p(base + o), nin, None) == E and "overlaps" in err(), (kind, i, o)
                assert L.pcx_repack_process(h, C.c_void_p(base + i), C.c_void_p(base + o), nin) == E and "overlaps" in err(), (kind, i, o)
            assert L.pcx_repack_set_bit_order(h, 0) == 0 and L.pcx_repack_get_bit_order(h, C.byref(msb)) == 0 and msb.value == 0
            assert L.pcx_repack_set_bit_order(h, 7) == 0 and L.pcx_repack_get_bit_order(h, C.byref(msb)) == 0 and msb.value == 1
        finally:
            assert L.pcx_repack_destroy(h) == 0
    assert L.pcx_repack_destroy(None) == 0


def test_overlap_refusals_name_the_kind_and_come_before_any_device_call(pcx):
    """The rule of in and out on fabricated addresses, which are never dereferenced: no kind works in place, so every shared byte is
    refused -- the same buffer, out one element into in, one byte shared at either end -- with the kind's own text, by the host and
    the device entry point alike."""
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    err = pcx._lib.last_error
    base = 1 << 40
    texts = {"bits_to_symbols": "bits to symbols", "symbols_to_bits": "symbols to bits", "bytes_to_symbols": "bytes to symbols",
             "symbols_to_bytes": "symbols to bytes"}
    for ki, kind in enumerate(M.KINDS):
        h = C.c_void_p()
        assert L.pcx_repack_create(ki, C.byref(h)) == 0
        try:
            assert L.pcx_repack_set_modulus(h, 3) == 0
            gin, gout = M.group(kind, 3)
            nin, nout = (1 << 18) * gin, (1 << 18) * gout
            text = texts[kind] + ": out overlaps in"
            for out in (base, base + 1, base + nin - 1, base - nout + 1):
                assert L.pcx_repack_process_dev(h, C.c_void_p(base), C.c_void_p(out), nin, None) == E and err() == text, (kind, out - base)
                assert L.pcx_repack_process(h, C.c_void_p(base), C.c_void_p(out), nin) == E and err() == text, (kind, out - base)
        finally:
            assert L.pcx_repack_destroy(h) == 0


def test_handle_reports_groups_and_geometry_at_every_setting(dev):
    for kind in M.KINDS:
        r = dev.SymbolRepacker(kind)
        assert (r.modulus(), r.bit_order()) == (1, M.FRESH_ORDER[kind])
        for w in M.WIDTHS:
            r.set_modulus(w)
            assert r.modulus() == w and r.group() == M.group(kind, w)
            tile, slc = r.geometry()
            gin = r.group()[0]
            assert tile % gin == 0 and tile % 16 == 0 and slc % tile == 0 and 0 < slc <= 64 << 20 and slc + tile > 64 << 20
            assert r.out_elems(tile) % 16 == 0
        for bad in (0, 9, -1, 1 << 40):
            with pytest.raises(ValueError, match="Modulus must be between 1 and 8 inclusive"):
                r.set_modulus(bad)
        assert r.modulus() == 8
        with pytest.raises(ValueError, match="Order must be LSBit or MSBit"):
            r.set_bit_order("msbit")
        r.set_bit_order("LSBit")
        assert r.bit_order() == "LSBit"
        assert r.process(np.zeros(0, np.uint8)).size == 0
        r.close()
    r = dev.SymbolRepacker("symbols_to_bytes", 3, "MSBit")
    assert (r.modulus(), r.bit_order()) == (3, "MSBit")
    with pytest.raises(ValueError, match="not a whole group"):
        r.process(np.zeros(7, np.uint8))
    r.close()
    with pytest.raises(ValueError, match="unknown kind"):
        dev.SymbolRepacker("bits_to_bytes")


def test_header_declares_the_family_and_the_binding_covers_it(pcx):
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    names = ("create", "destroy", "set_modulus", "get_modulus", "set_bit_order", "get_bit_order", "get_group", "get_geometry", "process",
             "process_dev")
    family = sorted(set(re.findall(r"PCX_API\s+int\s+(pcx_repack_\w+)\s*\(", src)))
    assert family == sorted("pcx_repack_" + n for n in names)
    assert sorted(n for n in pcx._lib.SIGNATURES if n.startswith("pcx_repack_")) == family
    enum = re.search(r"enum \{ (PCX_REPACK_BITS_TO_SYMBOLS[^}]*)\}", src).group(1)
    assert re.sub(r"\s+", " ", enum).strip() == ("PCX_REPACK_BITS_TO_SYMBOLS = 0, PCX_REPACK_SYMBOLS_TO_BITS = 1, "
                                                  "PCX_REPACK_BYTES_TO_SYMBOLS = 2, PCX_REPACK_SYMBOLS_TO_BYTES = 3")
    L = pcx._lib
    assert (L.REPACK_BITS_TO_SYMBOLS, L.REPACK_SYMBOLS_TO_BITS, L.REPACK_BYTES_TO_SYMBOLS, L.REPACK_SYMBOLS_TO_BYTES) == (0, 1, 2, 3)
    for text in ("msgWork", "not a whole group", "Modulus must be between 1 and 8 inclusive"):
        assert text in src


# ---- the blocks (libpcx_repack_blocks.so)
def test_module_registry_holds_exactly_the_eight_paths():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("repack") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="repack") == 0
        assert path not in B.registry_paths()
        for other in ("filter", "envelope", "iir", "digital", "correlator", "symbol"):
            assert path not in B.module_registry_paths(other)


def test_fresh_blocks_answer_the_constructors_values_and_refuse_what_the_reference_refuses():
    from pothoscomms_amd import _lib, blocks as B
    for prefix in ("/comms/", "/blocks/"):
        for kind in M.KINDS:
            b = B.make(prefix + kind, module="repack")
            assert (b.in_dtype, b.out_dtype) == ("uint8", "uint8")
            assert b.calls() == dict(COMMON_CALLS, **OWN_CALLS)
            assert (b.call("getModulus"), b.call("getBitOrder")) == (1, M.FRESH_ORDER[kind])
            b.call("setModulus", 5)
            for bad in (0, 9, 256 + 5, 1 << 32):
                with pytest.raises(_lib.InvalidArgument, match="Modulus must be between 1 and 8 inclusive"):
                    b.call("setModulus", bad)
            assert b.call("getModulus") == 5
            for order in ("MSBit", "LSBit"):
                b.call("setBitOrder", order)
                assert b.call("getBitOrder") == order
            for bad in ("", "msbit", "MSB", "LSBit "):
                with pytest.raises(_lib.InvalidArgument, match="Order must be LSBit or MSBit"):
                    b.call("setBitOrder", bad)
            assert b.call("getBitOrder") == "LSBit" and b.call("getPortSlabBytes") == 64 << 20
            b.close()


def test_a_work_call_with_nothing_to_do_sets_the_reserve_and_touches_nothing():
    from pothoscomms_amd import blocks as B
    for kind in M.KINDS:
        for w in (1, 3, 6, 8):
            b = B.make("/comms/" + kind, module="repack")
            b.call("setModulus", w)
            gin, gout = M.group(kind, w)
            # no input; less than a group of input; no room for a group of output
            for x, room in ((np.zeros(0, np.uint8), 64), (np.zeros(gin - 1, np.uint8), 64), (np.zeros(4 * gin, np.uint8), gout - 1)):
                out, consumed, produced, reserve, posted = b.work(x, room, labels=[B.Label("a", 0)] if x.size else ())
                assert (out.size, consumed, produced, reserve) == (0, 0, 0, M.reserve(kind, w)), (kind, w, x.size, room)
            b.close()


def _docs():
    return {d["factory"][0].split("/")[2]: d for d in parse_docs(open(SRC).read())}


def test_descriptions_match_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert sorted(d["factory"] for d in docs) == sorted(("/comms/" + n, []) for n in M.KINDS)
    calls = registered_calls(text)
    assert calls == set(COMMON_CALLS) | set(OWN_CALLS)
    for name, d in _docs().items():
        pairs = set()
        for kind, fn, keys in d["calls"]:
            assert fn in calls and len(keys) == 1, fn
            pairs.add((keys[0], fn, kind))
        assert pairs == {("N", "setModulus", "setter"), ("bitOrder", "setBitOrder", "setter"), ("device", "setDevice", "initializer"),
                         ("portSlabBytes", "setPortSlabBytes", "initializer")}, name
        assert set(d["params"]) == {k for k, _, _ in pairs}
        assert d["alias"] == ["/blocks/" + name] and d["category"] == ["/Digital", "/Symbol"]
        for key, p in d["params"].items():
            assert " ".join(p["desc"]).strip() and p["default"] is not None, (name, key)
            if p["options"]:
                assert p["default"] in p["options"]
        assert d["params"]["bitOrder"]["options"] == ['"MSBit"', '"LSBit"'] and d["params"]["N"]["widget"] == "SpinBox(minimum=1, maximum=8)"
        assert " ".join(d["prose"]).strip()


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_descriptions_have_the_reference_schema_and_their_own_words():
    for name, ours in _docs().items():
        ref = parse_docs(open(os.path.join(REF, "digital", REF_FILES[name])).read())[0]
        assert ours["title"] == ref["title"] and ours["factory"] == ref["factory"] and ours["category"] == ref["category"], name
        assert ours["alias"] == ref["alias"] and ours["keywords"] == ref["keywords"], name
        ext = {"device", "portSlabBytes"}
        assert [k for k in ours["order"] if k not in ext] == ref["order"], name
        assert {(fn, tuple(k), kind) for kind, fn, k in ours["calls"] if k[0] not in ext} == {(fn, tuple(k), kind) for kind, fn, k in ref["calls"]}
        for key, rp in ref["params"].items():
            for field in ("name", "default", "options", "widget", "preview", "tab", "units"):
                assert ours["params"][key][field] == rp[field], (name, key, field)

        def sentences(doc):
            text = " ".join(doc["prose"]) + " " + " ".join(" ".join(p["desc"]) for p in doc["params"].values())
            text = re.sub(r"<[^>]+>", " ", text)
            return {re.sub(r"\s+", " ", s).strip().lower() for s in re.split(r"[.;:]\s", text) if len(s.split()) >= 6}
        assert sentences(ours) and not (sentences(ours) & sentences(ref)), name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_source_type_checks_against_the_pothos_surface():
    blocks = os.path.dirname(SRC)
    flags = ["-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-DPCX_WITH_POTHOS",
             "-I" + os.path.join(ROOT, "tests", "pothos_decl"), "-I" + os.path.join(ROOT, "include"), "-I" + blocks]
    r = subprocess.run(["g++"] + flags + [SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_port_slab_default_is_the_one_of_the_other_modules():
    blocks = os.path.dirname(SRC)
    pat = r"constexpr size_t kPortSlabBytes = (\d+)u << (\d+);"
    a = re.search(pat, open(os.path.join(blocks, "comms_blocks.cpp")).read())
    b = re.search(pat, open(SRC).read())
    assert a and b and int(a.group(1)) << int(a.group(2)) == int(b.group(1)) << int(b.group(2))
    for d in parse_docs(open(SRC).read()):
        assert int(d["params"]["portSlabBytes"]["default"]) == int(a.group(1)) << int(a.group(2))


def test_the_deviation_is_written_down():
    for path in (os.path.join(ROOT, "INTEGRATION.md"), os.path.join(ROOT, "include", "pcx.h"), SRC):
        assert "msgWork" in open(path).read(), path
