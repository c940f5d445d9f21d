"""CPU suite of /comms/threshold: the two formulations of the model (tests/threshold_model.py) against each other and against the
recorded labels of the reference's loop (tests/golden/threshold.npz), the alternation rule of the C ABI's single index list, the C
ABI's argument checks, the registry of libpcx_utility_blocks.so, the block's description and its defaults.  No device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import threshold_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "utility_blocks.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "threshold.npz")
REF = "/root/reference"
PATHS = ["/blocks/threshold", "/comms/threshold"]
LEVELS = [(40, -25), (0, 0), (-25, 40), (7, 7), (-3, -2)]       # activation above, equal to and below the deactivation level
CALLS = {"setActivationLevel": 1, "getActivationLevel": 0, "setDeactivationLevel": 1, "getDeactivationLevel": 0, "setActivationId": 1,
         "getActivationId": 0, "setDeactivationId": 1, "getDeactivationId": 0, "setDevice": 1, "getDevice": 0, "setPortSlabBytes": 1,
         "getPortSlabBytes": 0}


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    cases = sorted(k[4:] for k in g.files if k.startswith("idx/"))
    assert len(cases) == 6 * 3 * 4 + 4
    return g, cases


@pytest.mark.parametrize("dtype", M.TYPES)
def test_the_two_formulations_agree_on_random_streams(dtype):
    rng = np.random.default_rng(50 + M.TYPES.index(dtype))
    for act, deact in LEVELS:
        for span in (3, 60, 120):
            x = rng.uniform(min(act, deact) - span, max(act, deact) + span, 3000)
            x = (x if "float" in dtype else np.rint(x)).astype(dtype)
            for entry in (0, 1):
                a, b = M.states_loop(x, act, deact, entry), M.states_scan(x, act, deact, entry)
                assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b), (dtype, act, deact, span, entry)
    # the four maps one after the other: keep, set, keep, toggle, toggle, clear, toggle
    x = np.array([0, 50, 0, 0, 0, -50, 0], dtype)
    for f in (M.states_loop, M.states_scan):
        assert list(f(x, -25, 40, 0)) == [1, 1, 0, 1, 0, 0, 1] and list(f(x, -25, 40, 1)) == [0, 1, 0, 1, 0, 0, 1]
        assert list(f(x, 40, -25, 0)) == [0, 1, 1, 1, 1, 0, 0] and list(f(x, 40, -25, 1)) == [1, 1, 1, 1, 1, 0, 0]
        assert f(x[:0], 0, 0, 1).size == 0


def test_both_formulations_equal_every_recorded_case(golden):
    g, cases = golden
    cuts = [int(c) for c in g["cuts"]]
    for key in cases:
        x, lv = g["in/" + key], g["levels/" + key]
        assert x.dtype.name == key.split("/")[0] and lv.dtype == x.dtype and sum(cuts) == x.size
        for f in (M.states_loop, M.states_scan):
            idx, n, entry, final, _ = M.run(x, lv[0], lv[1], 0, f)
            assert np.array_equal(idx, g["idx/" + key]) and (n, entry, final) == (g["idx/" + key].size, 0, int(g["final/" + key])), (key, f.__name__)
            # fed in the recorded calls, the state carried: the same labels
            state = [0]

            def work(buf):
                i, _, _, state[0], _ = M.run(buf, lv[0], lv[1], state[0], f)
                return i
            assert np.array_equal(M.run_cuts(work, x, cuts), g["idx/" + key]) and state[0] == int(g["final/" + key]), (key, f.__name__)
    # the recording holds what it is meant to: toggle bands with a label on every element, NaN levels without any activation
    assert all(g["idx/%s/below/band" % t].size == 300 for t in M.TYPES)
    assert all(g["idx/%s/nan_act/noise" % t].size == 0 for t in ("float64", "float32"))
    assert sum(g["idx/" + k].size > 0 for k in cases) >= 50


def test_kinds_alternate_from_the_entry_state_on_every_recorded_case(golden):
    g, cases = golden
    for key in cases:
        kind = g["kind/" + key]
        assert np.array_equal(kind, M.kinds(kind.size, 0)), key
        assert np.all(np.diff(g["idx/" + key].astype(np.int64)) > 0)
        # a stream entered active starts with a deactivation
        x, lv = g["in/" + key], g["levels/" + key]
        idx1, n1, _, _, s1 = M.run(x, lv[0], lv[1], 1)
        a, d = M.flags(x, lv[0], lv[1])
        want = np.where(np.concatenate([[1], s1[:-1]]) == 1, 0, 1)[idx1.astype(np.int64)]       # what the loop posts: by the state in front
        assert np.array_equal(M.kinds(n1, 1), want), key
        assert np.all(np.where(want == 1, a[idx1.astype(np.int64)], d[idx1.astype(np.int64)]))


# ---- the C ABI (no device is touched)
def test_abi_argument_errors_come_before_any_device_call(pcx):
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    buf = (C.c_double * 8)()
    nt, st, tile, slc = C.c_size_t(7), C.c_int(7), C.c_size_t(), C.c_size_t()
    h = C.c_void_p()
    assert L.pcx_threshold_create(None, pcx._lib.F64) == E
    for bad in (pcx._lib.U64, pcx._lib.U32, pcx._lib.U16, pcx._lib.U8, -1, 10):
        assert L.pcx_threshold_create(C.byref(h), bad) == E and "unsupported type" in pcx._lib.last_error() and not h.value
    assert L.pcx_threshold_set_levels(None, buf, buf) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_threshold_get_levels(None, buf, buf) == E
    assert L.pcx_threshold_reset(None) == E and L.pcx_threshold_set_state(None, 1) == E and L.pcx_threshold_get_state(None, C.byref(st)) == E
    assert L.pcx_threshold_process(None, buf, 4, None, None, 0, C.byref(nt), C.byref(st)) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_threshold_process_dev(None, buf, 4, None, None, 0, buf, None) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_threshold_states(None, buf, 4, buf) == E and L.pcx_threshold_states_dev(None, buf, 4, buf, None) == E
    assert L.pcx_threshold_get_geometry(None, C.byref(slc)) == E and L.pcx_threshold_get_geometry(C.byref(tile), None) == E
    assert L.pcx_threshold_get_geometry(C.byref(tile), C.byref(slc)) == 0
    assert tile.value % 64 == 0 and slc.value % tile.value == 0 and slc.value <= 64 << 20

    for scalar in (pcx._lib.F64, pcx._lib.F32, pcx._lib.I64, pcx._lib.I32, pcx._lib.I16, pcx._lib.I8):
        assert L.pcx_threshold_create(C.byref(h), scalar) == 0
        try:
            # the constructor's values
            lv = (C.c_int64 * 2)(-1, -1)
            assert L.pcx_threshold_get_levels(h, C.byref(lv, 0), C.byref(lv, 8)) == 0
            es = {pcx._lib.F64: 8, pcx._lib.F32: 4, pcx._lib.I64: 8, pcx._lib.I32: 4, pcx._lib.I16: 2, pcx._lib.I8: 1}[scalar]
            assert bytes(lv)[:es] == bytes(es) and bytes(lv)[8:8 + es] == bytes(es) and bytes(lv)[es:8] == b"\xff" * (8 - es)
            assert L.pcx_threshold_set_levels(h, None, buf) == E and L.pcx_threshold_set_levels(h, buf, None) == E
            # null counts, null buffers, an index capacity without a buffer, overlap
            assert L.pcx_threshold_process(h, buf, 4, None, None, 0, None, C.byref(st)) == E and "null count" in pcx._lib.last_error()
            assert L.pcx_threshold_process(h, buf, 4, None, None, 0, C.byref(nt), None) == E
            assert L.pcx_threshold_process_dev(h, buf, 4, None, None, 0, None, None) == E and "null count" in pcx._lib.last_error()
            assert L.pcx_threshold_process(h, None, 4, None, None, 0, C.byref(nt), C.byref(st)) == E and "null buffer" in pcx._lib.last_error()
            assert L.pcx_threshold_process_dev(h, None, 4, None, None, 0, buf, None) == E and "null buffer" in pcx._lib.last_error()
            assert L.pcx_threshold_process(h, buf, 4, None, None, 2, C.byref(nt), C.byref(st)) == E and "null index buffer" in pcx._lib.last_error()
            assert L.pcx_threshold_process_dev(h, buf, 4, None, None, 2, buf, None) == E and "null index buffer" in pcx._lib.last_error()
            base = C.addressof(buf)
            for shift in (1, es, 4 * es - 1):
                assert L.pcx_threshold_process(h, buf, 4, C.c_void_p(base + shift), None, 0, C.byref(nt), C.byref(st)) == E
                assert "overlaps" in pcx._lib.last_error()
                assert L.pcx_threshold_process_dev(h, C.c_void_p(base + shift), 4, buf, None, 0, buf, None) == E and "overlaps" in pcx._lib.last_error()
            assert L.pcx_threshold_states(h, None, 4, buf) == E and L.pcx_threshold_states(h, buf, 4, None) == E
            assert L.pcx_threshold_states_dev(h, None, 4, buf, None) == E
            # nothing to do
            assert L.pcx_threshold_states(h, None, 0, None) == 0 and L.pcx_threshold_states_dev(h, None, 0, None, None) == 0
        finally:
            assert L.pcx_threshold_destroy(h) == 0
            h = C.c_void_p()


def test_levels_keep_every_bit_of_the_element_type(dev):
    t = dev.Threshold("int64", 2**62 + 1, -(2**63))
    assert [int(v) for v in t.levels()] == [2**62 + 1, -(2**63)] and t.levels()[0].dtype == np.int64
    t.close()
    t = dev.Threshold("float32", 0.1, np.nan)
    assert t.levels()[0] == np.float32(0.1) and np.isnan(t.levels()[1]) and t.levels()[0].dtype == np.float32
    t.close()
    t = dev.Threshold()
    assert t.dtype == "float64" and t.levels() == (0.0, 0.0) and dev.Threshold.geometry()[0] % 64 == 0
    t.close()
    t = dev.Threshold("int8", -128, 127)
    assert [int(v) for v in t.levels()] == [-128, 127]
    with pytest.raises(ValueError):
        t.process(np.zeros(4, np.int16))
    t.close()
    for bad in ("complex_float32", "uint8", "uint32"):
        with pytest.raises(ValueError):
            dev.Threshold(bad)


def test_header_declares_the_family_and_the_binding_covers_it(pcx):
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    family = sorted(set(re.findall(r"PCX_API\s+int\s+(pcx_threshold_\w+)\s*\(", src)))
    assert family == sorted("pcx_threshold_" + n for n in (
        "create", "destroy", "set_levels", "get_levels", "reset", "get_state", "set_state", "get_geometry", "process", "process_dev",
        "states", "states_dev"))
    for name in family:
        assert name in pcx._lib.SIGNATURES
    assert sorted(n for n in pcx._lib.SIGNATURES if n.startswith("pcx_threshold_")) == family
    out = subprocess.run(["nm", "-D", "--defined-only", pcx._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(family) <= {l.split()[-1] for l in out.splitlines() if " T " in l}


# ---- the block (libpcx_utility_blocks.so)
def test_module_registry_holds_the_two_paths_with_arity_1():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("utility") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="utility") == 1
        assert path not in B.registry_paths()
        for other in ("filter", "envelope", "iir", "digital", "correlator", "symbol", "repack", "waveform"):
            assert path not in B.module_registry_paths(other)


@pytest.mark.parametrize("dtype", M.TYPES)
def test_a_fresh_block_answers_the_constructors_values(dtype):
    from pothoscomms_amd import blocks as B
    info = None if "float" in dtype else np.iinfo(dtype)
    for path in PATHS:
        b = B.make(path, dtype, module="utility")
        assert (b.in_dtype, b.out_dtype, b.in_dim, b.out_dim) == (dtype, dtype, 1, 1)
        assert b.call("getActivationLevel") == 0 and b.call("getDeactivationLevel") == 0
        assert b.call("getActivationId") == "" and b.call("getDeactivationId") == ""
        assert b.calls() == CALLS
        hi, lo = (0.75, -1e30) if info is None else (info.max, info.min)
        b.call("setActivationLevel", hi)
        b.call("setDeactivationLevel", lo)
        want = (np.dtype(dtype).type(hi), np.dtype(dtype).type(lo))
        assert (b.call("getActivationLevel"), b.call("getDeactivationLevel")) == (want[0], want[1])
        b.call("setActivationId", "on")
        b.call("setDeactivationId", "off")
        assert (b.call("getActivationId"), b.call("getDeactivationId")) == ("on", "off")
        b.call("setActivationId", "")
        assert b.call("getActivationId") == ""
        # no elements: nothing is consumed
        out, consumed, produced, reserve, labels = b.work(np.zeros(0, dtype), 64)
        assert (out.size, consumed, produced, labels) == (0, 0, 0, [])
        b.close()


@pytest.mark.parametrize("dtype", ["complex_float32", "complex_int16", "uint8", "uint16", "uint32", "uint64"])
def test_an_unsupported_type_throws(dtype):
    from pothoscomms_amd import blocks as B
    for path in PATHS:
        with pytest.raises(ValueError, match="unsupported type"):
            B.make(path, dtype, module="utility")
    with pytest.raises(ValueError, match="unsupported type"):
        B.make(PATHS[1], "float32", dimension=2, module="utility")


def test_description_matches_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert [d["factory"] for d in docs] == [("/comms/threshold", ["dtype"])]
    calls = registered_calls(text)
    assert calls == set(CALLS)
    d = docs[0]
    pairs = set()
    for kind, fn, keys in d["calls"]:
        assert fn in calls and len(keys) == 1, fn
        pairs.add((keys[0], fn, kind))
    assert pairs == {("activationLevel", "setActivationLevel", "setter"), ("deactivationLevel", "setDeactivationLevel", "setter"),
                     ("activationId", "setActivationId", "setter"), ("deactivationId", "setDeactivationId", "setter"),
                     ("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
    assert set(d["params"]) == {k for k, _, _ in pairs} | {"dtype"}
    assert d["params"]["dtype"]["default"] == '"float64"' and d["params"]["activationId"]["default"] == '""'
    assert d["alias"] == ["/blocks/threshold"] and d["category"] == ["/Utility"]
    for p in d["params"].values():
        assert " ".join(p["desc"]).strip() and p["default"] is not None
    assert " ".join(d["prose"]).strip()


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_description_has_the_reference_schema_and_its_own_words():
    ours = parse_docs(open(SRC).read())[0]
    ref = parse_docs(open(os.path.join(REF, "utility", "Threshold.cpp")).read())[0]
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
    assert sentences(ours) and sentences(ref) and not (sentences(ours) & sentences(ref))


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
    assert int(parse_docs(open(SRC).read())[0]["params"]["portSlabBytes"]["default"]) == int(a.group(1)) << int(a.group(2))


def test_the_module_library_exports_the_runner_and_nothing_of_the_block():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_utility_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"pcxb_make", "pcxb_work", "pcxb_activate", "pcxb_call_int64", "pcxb_get_int64", "pcxb_call_double", "pcxb_get_double",
            "pcxb_call_string", "pcxb_get_string", "pcxb_registry_path"} <= exported
    assert all(s.startswith("pcxb_") for s in exported), sorted(s for s in exported if not s.startswith("pcxb_"))
