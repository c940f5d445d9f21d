"""CPU suite of /comms/scrambler and /comms/descrambler: the model (tests/scrambler_model.py) against the recorded reference outputs
(tests/golden/scrambler.npz), its plan rule, jump and window check, the C ABI's argument checks, the registry of
libpcx_digital_blocks.so and the two block descriptions."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import scrambler_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "digital_blocks.cpp")
REF = "/root/reference"
PATHS = ["/blocks/descrambler", "/blocks/scrambler", "/comms/descrambler", "/comms/scrambler"]
# polynomial, its top bit m: SCAN with any seed below 2^m
SCAN_POLYS = [(0x19, 4), (0x11021, 16), (0x8000000000000003, 63), (0x7, 2)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "scrambler.npz"))


def stream_of(golden, key):
    """(input bytes, recorded output bits) of a fixture case"""
    x = golden["in"]
    return x, np.unpackbits(golden["out/" + key])[:x.shape[0]]


def test_fixture_holds_the_whole_case_grid(golden):
    cases = list(golden["cases"])
    assert len(cases) == 2 * 2 * 11 and int(golden["cuts"].sum()) == golden["in"].shape[0] == 1000
    assert list(golden["cuts"][:4]) == [1, 37, 100, 11]
    assert golden["in"].max() > 1                                   # the upper bits of the input bytes are exercised
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "scrambler.npz")) < 100 << 10


def test_model_equals_the_recorded_reference_on_every_case(golden):
    for key in golden["cases"]:
        x, want = stream_of(golden, key)
        out, data, mask, _ = M.run_case(golden["cfg/" + key], golden["cuts"], x)
        assert np.array_equal(out, want), key
        assert (data, mask) == tuple(int(v) for v in golden["state/" + key]), key


def test_plan_rule_agrees_with_the_case_table(golden):
    serial = set()
    for key in golden["cases"]:
        cfg = golden["cfg/" + key]
        _, _, _, plan = M.run_case(cfg, golden["cuts"], golden["in"])
        assert plan == ("SERIAL" if cfg[6] else "SCAN"), key
        if cfg[6]:
            serial.add(key.split("/")[2])
    assert serial == {"p19_s10", "p19_sF3", "p19_sneg1", "p1_after_p19", "p0_after_p11021"}


def test_mask_is_every_bit_from_the_top_bit_upward_and_is_retained():
    l = M.glfsr_init(M.Lfsr(), 0x19, 1)
    assert (l.polynomial, l.data, l.mask) == (0x19, 1, 0xFFFFFFFFFFFFFFF0)
    M.glfsr_init(l, 1, 1)
    assert (l.polynomial, l.mask) == (1, 0xFFFFFFFFFFFFFFF0) and M.plan(l) == "SERIAL"
    M.glfsr_init(l, 0, 7)
    assert (l.polynomial, l.data, l.mask) == (1, 7, 0xFFFFFFFFFFFFFFF0)
    assert M.glfsr_init(M.Lfsr(), 0x8000000000000003, 5).mask == 1 << 63
    assert M.glfsr_init(M.Lfsr(), -0x7FFFFFFFFFFFFFFD, 5).mask == 1 << 63            # the same polynomial as an int64_t
    assert M.glfsr_init(M.Lfsr(), 2, 1).mask == 0xFFFFFFFFFFFFFFFE
    for poly, m in SCAN_POLYS:
        assert M.lowest_bit(M.glfsr_init(M.Lfsr(), poly, 1).mask) == m


@pytest.mark.parametrize("mode", ["additive", "multiplicative"])
def test_descrambling_with_equal_seeds_returns_the_input(mode):
    x = np.random.default_rng(1).integers(0, 256, 3000, dtype=np.uint8)
    for poly, m in SCAN_POLYS + [(0x80000D, 23)]:
        seed = 0x2A5A5A & ((1 << m) - 1) | 1
        y = M.Model(False, mode, poly, seed).process(x)
        back = M.Model(True, mode, poly, seed).process(y)
        assert np.array_equal(back, x & 1), (mode, hex(poly))
        assert np.any(y != (x & 1))


def test_model_carries_its_register_across_calls():
    x = np.random.default_rng(2).integers(0, 256, 2000, dtype=np.uint8)
    for descramble in (False, True):
        for mode in ("additive", "multiplicative"):
            whole = M.Model(descramble, mode, 0x11021, 0xACE1).process(x)
            m = M.Model(descramble, mode, 0x11021, 0xACE1)
            parts = np.concatenate([m.process(x[a:b]) for a, b in ((0, 1), (1, 38), (38, 1000), (1000, 2000))])
            assert np.array_equal(whole, parts)


def test_window_check_has_no_false_alarm_and_finds_a_flipped_bit(golden):
    seen = 0
    for key in golden["cases"]:
        cfg = golden["cfg/" + key]
        if cfg[6] or cfg[2]:
            continue
        # the last call of a case runs from a fresh register: a stream of its own
        x, out = stream_of(golden, key)
        a = int(golden["cuts"][:4].sum())
        x, out = x[a:], out[a:]
        l = M.glfsr_init(M.Lfsr(), int(cfg[4]), int(cfg[5]))
        m = M.lowest_bit(l.mask)
        kind = M.kind_of(cfg[0], "multiplicative" if cfg[1] else "additive")
        assert M.window_check(x, out, l.polynomial, m, kind) == 0, key
        for at in (m + 3, 400, out.shape[0] - 1):
            bad = out.copy()
            bad[at] ^= 1
            assert M.window_check(x, bad, l.polynomial, m, kind) >= 1, (key, at)
        bad = out.copy()
        bad[400] ^= 1
        assert 2 <= M.window_check(x, bad, l.polynomial, m, kind) <= m + 1, key
        assert M.state_from_tail(x, out, l.polynomial, m, kind) == int(golden["state/" + key][0]), key
        seen += 1
    assert seen == 2 * 2 * 6


def test_window_check_on_torch_tensors_agrees_with_numpy():
    torch = pytest.importorskip("torch")
    x = np.random.default_rng(3).integers(0, 256, 5000, dtype=np.uint8)
    for poly, m in SCAN_POLYS:
        for kind, (descramble, mode) in (("additive", (False, "additive")), ("scrambler", (False, "multiplicative")),
                                         ("descrambler", (True, "multiplicative"))):
            mod = M.Model(descramble, mode, poly, 1)
            out = mod.process(x)
            bad = out.copy()
            bad[2500] ^= 1
            pol = M.u64(poly) | 1
            assert M.window_check(torch.from_numpy(x), torch.from_numpy(out), pol, m, kind, piece=1024) == 0
            assert M.window_check(torch.from_numpy(x), torch.from_numpy(bad), pol, m, kind, piece=1024) == M.window_check(x, bad, pol, m, kind) >= 1
            assert M.state_from_tail(torch.from_numpy(x), torch.from_numpy(out), pol, m, kind) == mod.l.data


def test_jump_equals_stepping():
    for poly, m in SCAN_POLYS:
        pol = M.u64(poly) | 1
        mod = M.Model(False, "additive", poly, 1)
        at = 0
        for n in (0, 1, 2, 63, 64, 1000, 4097):
            mod.process(np.zeros(n - at, np.uint8))
            at = n
            assert M.jump(1, n, pol, m) == mod.l.data, (hex(poly), n)
        assert M.jump(M.jump(1, 12345, pol, m), 1 << 33, pol, m) == M.jump(1, 12345 + (1 << 33), pol, m)


# ---- the C ABI (no device is touched: the mode and the handle are checked first)
def test_abi_refuses_a_bad_mode_or_handle_before_touching_the_device(pcx):
    L = pcx._lib.load()
    for mode in (-1, 2, 99):
        assert L.pcx_scrambler_set_mode(None, mode) == pcx._lib.ERR_ARG and "unknown mode" in pcx._lib.last_error()
    assert L.pcx_scrambler_set_mode(None, pcx._lib.SCR_ADDITIVE) == pcx._lib.ERR_ARG and "null handle" in pcx._lib.last_error()
    assert L.pcx_scrambler_set_poly(None, 0x19) == pcx._lib.ERR_ARG
    assert L.pcx_scrambler_set_seed(None, 1) == pcx._lib.ERR_ARG
    assert L.pcx_scrambler_process(None, None, None, 1) == pcx._lib.ERR_ARG
    assert L.pcx_scrambler_process_dev(None, None, None, 1, None) == pcx._lib.ERR_ARG
    v, w = C.c_int(), C.c_int64()
    assert L.pcx_scrambler_get_plan(None, C.byref(v)) == pcx._lib.ERR_ARG
    assert L.pcx_scrambler_get_mode(None, C.byref(v)) == pcx._lib.ERR_ARG
    assert L.pcx_scrambler_get_poly(None, C.byref(w)) == pcx._lib.ERR_ARG
    assert L.pcx_scrambler_get_state(None, C.byref(w), C.byref(w)) == pcx._lib.ERR_ARG
    assert L.pcx_scrambler_create(0, None) == pcx._lib.ERR_ARG


def test_geometry_nests(dev):
    run, tile, group, slc = dev.Scrambler.geometry()
    assert run % 64 == 0 and tile % run == 0 and group % tile == 0 and slc % group == 0 and slc <= 64 << 20


# ---- the blocks (libpcx_digital_blocks.so)
def test_module_registry_holds_the_four_paths_with_arity_0():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("digital") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="digital") == 0
        assert path not in B.registry_paths()
        for other in ("filter", "envelope", "iir"):
            assert path not in B.module_registry_paths(other)


def test_descriptions_match_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert [d["factory"] for d in docs] == [("/comms/scrambler", []), ("/comms/descrambler", [])]
    calls = registered_calls(text)
    assert calls == {"setPoly", "poly", "setSeed", "seed", "setMode", "mode", "setSync", "sync", "setDevice", "getDevice",
                     "setPortSlabBytes", "getPortSlabBytes"}
    for d, name in zip(docs, ("scrambler", "descrambler")):
        pairs = set()
        for kind, fn, keys in d["calls"]:
            assert fn in calls and len(keys) == 1, fn
            pairs.add((keys[0], fn, kind))
        assert pairs == {("poly", "setPoly", "setter"), ("mode", "setMode", "setter"), ("seed", "setSeed", "setter"),
                         ("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
        assert set(d["params"]) == {k for k, _, _ in pairs}
        assert d["params"]["mode"]["default"] == '"multiplicative"' and d["params"]["mode"]["options"] == ['"additive"', '"multiplicative"']
        assert d["params"]["poly"]["default"] == "0x19" and d["params"]["seed"]["default"] == "0x1"
        assert d["alias"] == ["/blocks/" + name] and d["category"] == ["/Digital"]
        for p in d["params"].values():
            assert " ".join(p["desc"]).strip()
        assert " ".join(d["prose"]).strip()


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_descriptions_have_the_reference_schema_and_their_own_words():
    import re
    for ours, name in zip(parse_docs(open(SRC).read()), ("Scrambler.cpp", "Descrambler.cpp")):
        ref = parse_docs(open(os.path.join(REF, "digital", name)).read())[0]
        assert ours["title"] == ref["title"] and ours["factory"] == ref["factory"] and ours["category"] == ref["category"]
        assert ours["alias"] == ref["alias"] and ours["keywords"] == ref["keywords"]
        ext = {"device", "portSlabBytes"}
        assert [k for k in ours["order"] if k not in ext] == ref["order"]
        assert {(fn, tuple(k), kind) for kind, fn, k in ours["calls"] if k[0] not in ext} == {(fn, tuple(k), kind) for kind, fn, k in ref["calls"]}
        for key, rp in ref["params"].items():
            for field in ("name", "default", "options", "widget", "preview", "tab", "units"):
                assert ours["params"][key][field] == rp[field], (key, field)

        def sentences(doc):
            text = " ".join(doc["prose"]) + " " + " ".join(" ".join(p["desc"]) for p in doc["params"].values())
            text = re.sub(r"<[^>]+>", " ", text)
            return {re.sub(r"\s+", " ", s).strip().lower() for s in re.split(r"[.;:]\s", text) if len(s.split()) >= 6}
        assert not (sentences(ours) & sentences(ref))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_source_type_checks_against_the_pothos_surface():
    blocks = os.path.dirname(SRC)
    flags = ["-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-DPCX_WITH_POTHOS",
             "-I" + os.path.join(ROOT, "tests", "pothos_decl"), "-I" + os.path.join(ROOT, "include"), "-I" + blocks]
    r = subprocess.run(["g++"] + flags + [SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_port_slab_default_is_the_one_of_the_other_modules():
    import re
    blocks = os.path.dirname(SRC)
    pat = r"constexpr size_t kPortSlabBytes = (\d+)u << (\d+);"
    a = re.search(pat, open(os.path.join(blocks, "comms_blocks.cpp")).read())
    b = re.search(pat, open(SRC).read())
    assert a and b and int(a.group(1)) << int(a.group(2)) == int(b.group(1)) << int(b.group(2))
    for d in parse_docs(open(SRC).read()):
        assert int(d["params"]["portSlabBytes"]["default"]) == int(a.group(1)) << int(a.group(2))


def test_runner_header_declares_the_int64_call_and_getter():
    src = open(os.path.join(ROOT, "include", "pcx_blocks.h")).read()
    assert "pcxb_call_int64" in src and "pcxb_get_int64" in src
