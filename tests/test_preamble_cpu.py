"""CPU suite of /comms/preamble_correlator: the two formulations of the model (tests/preamble_model.py) against each other, the one
scenario the reference's own test fixes, the C ABI's argument checks, the registry of libpcx_correlator_blocks.so, the block's
description and its defaults.  No device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import preamble_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "correlator_blocks.cpp")
REF = "/root/reference"
PATHS = ["/blocks/preamble_correlator", "/comms/preamble_correlator"]
LENGTHS = [1, 2, 6, 31, 32, 33, 64, 65, 255, 1024]


def thresholds(P):
    return sorted({0, 1, P, 8 * P - 1, 8 * P})


@pytest.mark.parametrize("P", LENGTHS)
def test_the_two_formulations_agree_on_random_bytes(P):
    rng = np.random.default_rng(100 + P)
    for width in (1, 3, 8):
        pre = rng.integers(0, 1 << width, P, dtype=np.uint8)
        x = rng.integers(0, 256, 5 * P + 700, dtype=np.uint8)
        x = M.plant(x, pre, [0, 2 * P + 13, x.size - P - 1])
        d = M.distances_plain(pre, x)
        assert d.size == x.size - P and np.array_equal(d, M.distances_planes(pre, x)), (P, width)
        assert d[0] == 0 and d[2 * P + 13] == 0 and d[-1] == 0 and int(d.max()) <= 8 * P
        for thr in thresholds(P):
            a, b = M.matches_plain(pre, thr, x), M.matches_planes(pre, thr, x)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (P, width, thr)
            assert a[2] >= 3
            if thr == 8 * P:
                assert a[2] == a[1] and np.array_equal(a[0], np.arange(P, x.size, dtype=np.uint64))


def test_torch_formulation_agrees_in_chunks():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7)
    for P, width in ((6, 1), (33, 2), (64, 8), (255, 1)):
        pre = rng.integers(0, 1 << width, P, dtype=np.uint8)
        x = M.plant(rng.integers(0, 256, 5000, dtype=np.uint8), pre, [0, 1234, 5000 - P - 1])
        d = M.distances_plain(pre, x)
        idx, N, nm = M.matches_plain(pre, P, x)
        xt = torch.from_numpy(x)
        got = M.torch_check(pre, P, xt, dist=torch.from_numpy(d.astype(np.int64)), idx=torch.from_numpy(idx.astype(np.int64)), chunk=999)
        assert got == (N, nm, 0, 0), (P, got)
        wrong = d.astype(np.int64)
        wrong[1000] += 1
        assert M.torch_check(pre, P, xt, dist=torch.from_numpy(wrong), chunk=999)[2] == 1
        assert M.torch_check(pre, P, xt, idx=torch.from_numpy(idx[:-1].astype(np.int64)), chunk=999)[3] >= 1


def reference_scenario():
    """TestPreambleCorrelator.cpp:16-27: 16 alternating symbols, the preamble planted at 4, and a preamble-sized tail, which the
    reference leaves unset and which is zero here"""
    pre = np.array([0, 1, 1, 1, 1, 0], np.uint8)
    x = np.zeros(16 + 6, np.uint8)
    x[:16] = np.arange(16) % 2
    x[4:10] = pre
    return pre, x


def test_the_reference_tests_own_scenario():
    pre, x = reference_scenario()
    for thr, want in ((0, [10]), (1, [10]), (2, [8, 10, 11, 15, 18])):
        for f in (M.matches_plain, M.matches_planes):
            idx, N, nm = f(pre, thr, x)
            assert (list(idx), N, nm) == (want, 16, len(want)), (thr, f.__name__)


def test_dirty_upper_bits_never_match_a_bit_preamble_at_threshold_0():
    rng = np.random.default_rng(3)
    pre = rng.integers(0, 2, 24, dtype=np.uint8)
    bits = M.plant(rng.integers(0, 2, 600, dtype=np.uint8), pre, [100, 400])
    clean = M.matches_plain(pre, 0, bits)[0]
    assert {124, 424} <= set(int(i) for i in clean)
    dirty = bits | 0x80
    for f in (M.matches_plain, M.matches_planes):
        assert f(pre, 0, dirty)[2] == 0
        assert f(pre, 23, dirty)[2] == 0                 # every symbol of the window carries one wrong bit
        assert np.array_equal(f(pre, 24, dirty)[0], clean)
    assert np.array_equal(M.distances_plain(pre, dirty), M.distances_plain(pre, bits) + 24)


def test_no_positions_up_to_the_preambles_length():
    pre = np.arange(1, 8, dtype=np.uint8)
    for n in (0, 1, 6, 7):
        for f in (M.matches_plain, M.matches_planes):
            idx, N, nm = f(pre, 100, np.zeros(n, np.uint8))
            assert (idx.size, N, nm) == (0, 0, 0)
    assert M.matches_plain(pre, 100, np.zeros(8, np.uint8))[1:] == (1, 1)
    with pytest.raises(ValueError):
        M.distances_plain([], np.zeros(4, np.uint8))


def test_run_cuts_equals_the_one_shot_model():
    rng = np.random.default_rng(4)
    pre = rng.integers(0, 2, 9, dtype=np.uint8)
    x = M.plant(rng.integers(0, 2, 400, dtype=np.uint8), pre, [0, 95, 200, 391])

    def work(buf):
        idx, N, _ = M.matches_plain(pre, 1, buf)
        return N, idx
    labels, done = M.run_cuts(work, x, [3, 9, 10, 100, 1, 277], pre.size)
    want = M.matches_plain(pre, 1, x)
    assert done == want[1] and np.array_equal(labels, want[0])


# ---- the C ABI (no device is touched)
def test_abi_argument_errors_come_before_any_device_call(pcx):
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    one = (C.c_ubyte * 1)(1)
    npos, nm, n, t, p = C.c_size_t(7), C.c_size_t(7), C.c_size_t(), C.c_uint(), C.c_int()
    assert L.pcx_preamble_create(None) == E
    assert L.pcx_preamble_set_preamble(None, one, 0) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_preamble_set_preamble(None, one, 1) == E
    assert L.pcx_preamble_set_threshold(None, 1) == E
    assert L.pcx_preamble_get_threshold(None, C.byref(t)) == E
    assert L.pcx_preamble_get_plan(None, C.byref(p)) == E
    assert L.pcx_preamble_get_preamble(None, None, 0, C.byref(n)) == E
    assert L.pcx_preamble_process(None, None, 10, None, None, 0, C.byref(npos), C.byref(nm)) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_preamble_process_dev(None, None, 10, None, None, 0, None, None, None) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_preamble_distances(None, None, 10, None, C.byref(npos)) == E
    assert L.pcx_preamble_distances_dev(None, None, 10, None, None) == E
    assert L.pcx_preamble_get_geometry(None, None, None) == E

    h = C.c_void_p()
    assert L.pcx_preamble_create(C.byref(h)) == 0
    try:
        # the constructor's values
        assert L.pcx_preamble_get_threshold(h, C.byref(t)) == 0 and t.value == 1
        buf = (C.c_ubyte * 4)()
        assert L.pcx_preamble_get_preamble(h, buf, 4, C.byref(n)) == 0 and (n.value, buf[0]) == (1, 1)
        assert L.pcx_preamble_get_plan(h, C.byref(p)) == 0 and p.value == pcx._lib.PRE_PLANES
        # empty preamble, then null counts
        assert L.pcx_preamble_set_preamble(h, one, 0) == E and "preamble cannot be empty" in pcx._lib.last_error()
        assert L.pcx_preamble_set_preamble(h, None, 0) == E and "preamble cannot be empty" in pcx._lib.last_error()
        assert L.pcx_preamble_set_preamble(h, None, 3) == E
        assert L.pcx_preamble_get_preamble(h, buf, 4, C.byref(n)) == 0 and (n.value, buf[0]) == (1, 1)      # refused: unchanged
        assert L.pcx_preamble_process(h, one, 10, None, None, 0, None, C.byref(nm)) == E and "null count" in pcx._lib.last_error()
        assert L.pcx_preamble_process(h, one, 10, None, None, 0, C.byref(npos), None) == E
        assert L.pcx_preamble_process_dev(h, one, 10, None, None, 0, None, None, None) == E and "null count" in pcx._lib.last_error()
        assert L.pcx_preamble_distances(h, one, 10, None, None) == E and "null count" in pcx._lib.last_error()
        # n_in <= P: no positions, nothing to compute
        assert L.pcx_preamble_process(h, one, 1, None, None, 0, C.byref(npos), C.byref(nm)) == 0 and (npos.value, nm.value) == (0, 0)
        npos.value = 7
        assert L.pcx_preamble_process(h, None, 0, None, None, 0, C.byref(npos), C.byref(nm)) == 0 and npos.value == 0
        npos.value = 7
        assert L.pcx_preamble_distances(h, one, 1, None, C.byref(npos)) == 0 and npos.value == 0
        assert L.pcx_preamble_distances_dev(h, None, 1, None, None) == 0
        # null buffers once there are positions
        assert L.pcx_preamble_process(h, None, 10, None, None, 0, C.byref(npos), C.byref(nm)) == E and "null buffer" in pcx._lib.last_error()
        idx = (C.c_uint64 * 2)()
        assert L.pcx_preamble_process(h, one, 10, None, None, 2, C.byref(npos), C.byref(nm)) == E and "null index buffer" in pcx._lib.last_error()
        assert L.pcx_preamble_process_dev(h, None, 10, None, idx, 2, idx, idx, None) == E and "null buffer" in pcx._lib.last_error()
        assert L.pcx_preamble_distances(h, one, 10, None, C.byref(npos)) == E
        assert L.pcx_preamble_set_threshold(h, 0xFFFFFFFF) == 0
        assert L.pcx_preamble_get_threshold(h, C.byref(t)) == 0 and t.value == 0xFFFFFFFF
    finally:
        assert L.pcx_preamble_destroy(h) == 0


def test_plan_follows_the_preambles_length(dev):
    tile, slc, longest = dev.PreambleCorrelator.geometry()
    assert tile % 64 == 0 and slc % tile == 0 and slc <= 64 << 20 and longest >= 1024
    c = dev.PreambleCorrelator()
    assert (list(c.preamble()), c.threshold(), c.plan()) == ([1], 1, dev._lib.PRE_PLANES)
    c.set_preamble(np.arange(longest) % 251)
    assert c.plan() == dev._lib.PRE_PLANES and np.array_equal(c.preamble(), (np.arange(longest) % 251).astype(np.uint8))
    c.set_preamble(np.ones(longest + 1))
    assert c.plan() == dev._lib.PRE_BYTES
    with pytest.raises(ValueError, match="preamble cannot be empty"):
        c.set_preamble([])
    assert c.preamble().size == longest + 1
    idx, npos, nm = c.process(np.zeros(longest + 1, np.uint8))
    assert (idx.size, npos, nm) == (0, 0, 0) and c.distances(np.zeros(5, np.uint8)).size == 0
    c.close()


def test_header_declares_the_family_and_the_binding_covers_it(pcx):
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    family = sorted(set(re.findall(r"PCX_API\s+int\s+(pcx_preamble_\w+)\s*\(", src)))
    assert family == sorted("pcx_preamble_" + n for n in (
        "create", "destroy", "set_preamble", "get_preamble", "set_threshold", "get_threshold", "get_plan", "get_geometry", "process",
        "process_dev", "distances", "distances_dev"))
    for name in family:
        assert name in pcx._lib.SIGNATURES
    assert sorted(n for n in pcx._lib.SIGNATURES if n.startswith("pcx_preamble_")) == family


# ---- the block (libpcx_correlator_blocks.so)
def test_module_registry_holds_the_two_paths_with_arity_0():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("correlator") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="correlator") == 0
        assert path not in B.registry_paths()
        for other in ("filter", "envelope", "iir", "digital"):
            assert path not in B.module_registry_paths(other)


def test_a_fresh_block_answers_the_constructors_values():
    from pothoscomms_amd import blocks as B
    for path in PATHS:
        b = B.make(path, module="correlator")
        assert b.call("getThreshold") == 1 and b.call("getPreamble") == [1] and b.call("getFrameStartId") == "frameStart"
        assert (b.in_dtype, b.out_dtype) == ("uint8", "uint8")
        b.call("setPreamble", [0, 1, 1, 1, 1, 0])
        b.call("setThreshold", 2)
        b.call("setFrameStartId", "sof")
        assert b.call("getThreshold") == 2 and b.call("getPreamble") == [0, 1, 1, 1, 1, 0] and b.call("getFrameStartId") == "sof"
        with pytest.raises(ValueError, match="preamble cannot be empty"):
            b.call("setPreamble", [])
        assert b.call("getPreamble") == [0, 1, 1, 1, 1, 0]
        assert b.calls() == {"setPreamble": 1, "getPreamble": 0, "setThreshold": 1, "getThreshold": 0, "setFrameStartId": 1,
                             "getFrameStartId": 0, "setDevice": 1, "getDevice": 0, "setPortSlabBytes": 1, "getPortSlabBytes": 0}
        # fewer elements than the preamble and one: nothing is consumed, the reserve is asked for all the same
        out, consumed, produced, reserve, labels = b.work(np.zeros(6, np.uint8), 64)
        assert (out.size, consumed, produced, reserve, labels) == (0, 0, 0, 7, [])
        b.close()


def test_description_matches_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert [d["factory"] for d in docs] == [("/comms/preamble_correlator", [])]
    calls = registered_calls(text)
    assert calls == {"setPreamble", "getPreamble", "setThreshold", "getThreshold", "setFrameStartId", "getFrameStartId", "setDevice",
                     "getDevice", "setPortSlabBytes", "getPortSlabBytes"}
    d = docs[0]
    pairs = set()
    for kind, fn, keys in d["calls"]:
        assert fn in calls and len(keys) == 1, fn
        pairs.add((keys[0], fn, kind))
    assert pairs == {("preamble", "setPreamble", "setter"), ("thresh", "setThreshold", "setter"),
                     ("frameStartId", "setFrameStartId", "setter"), ("device", "setDevice", "initializer"),
                     ("portSlabBytes", "setPortSlabBytes", "initializer")}
    assert set(d["params"]) == {k for k, _, _ in pairs}
    assert d["params"]["preamble"]["default"] == "[1]" and d["params"]["frameStartId"]["default"] == '"frameStart"'
    assert d["alias"] == ["/blocks/preamble_correlator"] and d["category"] == ["/Digital"]
    for p in d["params"].values():
        assert " ".join(p["desc"]).strip() and p["default"] is not None
    assert " ".join(d["prose"]).strip()


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_description_has_the_reference_schema_and_its_own_words():
    ours = parse_docs(open(SRC).read())[0]
    ref = parse_docs(open(os.path.join(REF, "digital", "PreambleCorrelator.cpp")).read())[0]
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


def test_runner_exports_the_byte_vector_call_in_every_module():
    src = open(os.path.join(ROOT, "include", "pcx_blocks.h")).read()
    assert "pcxb_call_bytes" in src and "pcxb_get_bytes" in src
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_correlator_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"pcxb_call_bytes", "pcxb_get_bytes", "pcxb_work"} <= exported


# ---- the recorded reference: tests/golden/preamble.npz, what the reference's own work() posted (tests/golden/make_preamble_golden.py)
GOLDEN = os.path.join(ROOT, "tests", "golden", "preamble.npz")
GOLDEN_LENGTHS = LENGTHS + [1027]


@pytest.fixture(scope="module")
def golden():
    return M.golden_cases(GOLDEN)


def test_model_equals_every_recorded_call_of_the_reference(golden):
    tile, halo, cases = golden
    ran = 0
    for c in cases:
        pre, x, P = c["preamble"], c["x"], c["preamble"].size
        if c["cuts"] is None:
            d = M.distances_plain(pre, x)
            assert np.array_equal(d, M.distances_planes(pre, x)), c["name"]
            for thr, handed, consumed, reserve, forwarded, idx in c["calls"]:
                want, N, nm = M.matches_plain(pre, thr, x)
                assert (handed, consumed, forwarded, reserve) == (x.size, N, N, P + 1), (c["name"], thr)
                assert nm == idx.size and np.array_equal(want, idx), (c["name"], thr)
        else:
            calls = iter(c["calls"])
            thr = c["calls"][0][0]

            def work(buf):
                t, handed, consumed, reserve, forwarded, idx = next(calls)
                want, N, nm = M.matches_plain(pre, thr, buf)
                assert (t, handed, consumed, forwarded, reserve) == (thr, buf.size, N, N, P + 1), c["name"]
                assert np.array_equal(want, idx), c["name"]
                return N, want
            labels, done = M.run_cuts(work, x, c["cuts"], P)
            assert next(calls, None) is None
            one_shot = M.matches_plain(pre, thr, x)
            assert done == one_shot[1] and np.array_equal(labels, one_shot[0]), c["name"]
        ran += 1
    assert ran == np.load(GOLDEN)["names"].size == len(cases)


def test_recorded_fixture_covers_what_it_is_meant_to(golden):
    tile, halo, cases = golden
    assert os.path.getsize(GOLDEN) <= 512 << 10
    assert (tile, halo) == (4096, 1024)
    by = {c["name"]: c for c in cases}
    assert len(by) == len(cases)
    for P in GOLDEN_LENGTHS:
        for width in (1, 8):
            c = by["grid/P%d/w%d" % (P, width)]
            x, at = c["x"], c["at"]
            assert c["preamble"].size == P and x.size == 3 * tile + 2 * P + 37 and int(x.max()) < 1 << width and int(c["preamble"].max()) < 1 << width
            d = M.distances_plain(c["preamble"], x)
            assert all(d[a] == 0 for a in at) and 0 in at and d.size - 1 in at            # every plant whole, the first and the last position
            if P >= 2:
                assert all(any(a < seam < a + P for a in at) for seam in (tile, 2 * tile)), P     # a plant across either seam
            assert any(a + P == 2 * tile - P - 1 for a in at) or P >= tile // 4                   # right in front of a seam's window
            assert [call[0] for call in c["calls"]] == sorted({0, 1, P, 8 * P - 1, 8 * P})
            first, last = c["calls"][0], c["calls"][-1]
            assert {a + P for a in at} <= set(first[5].tolist())                                  # threshold 0 finds the plants
            assert np.array_equal(last[5], np.arange(P, x.size, dtype=np.uint64))                 # threshold 8 P matches everywhere
            assert int(last[5][-1]) == x.size - 1 >= last[4] == x.size - P                        # labels run past the forwarded elements: no clamp
    assert 1027 > halo >= 1024
    for P in (6, 64, 257):
        for pname in ("random", "zero", "ones"):
            for fill in ("00", "ff"):
                c = by["fill/P%d/%s/%s" % (P, pname, fill)]
                assert c["x"].size == 2 * tile + P + 3 and c["x"].min() == c["x"].max() == int(fill, 16)
                counts = [call[5].size for call in c["calls"]]
                assert counts[-1] == c["x"].size - P and set(counts) <= {0, counts[-1]} and counts[0] in (0, counts[-1])
    for width in (1, 2, 4, 8):
        for P in (16, 100):
            for where in ("lo", "hi"):
                c, noisy = by["planes/w%d/P%d/%s" % (width, P, where)], by["planes/w%d/P%d/%s/noisy" % (width, P, where)]
                active = int(np.bitwise_or.reduce(c["preamble"]))
                assert bin(active).count("1") == width and (active & 1 if where == "lo" else active & 0x80)
                d, dn = M.distances_plain(c["preamble"], c["x"]), M.distances_plain(c["preamble"], noisy["x"])
                assert all(d[a] == 0 for a in c["at"]) and sorted(int(dn[a]) for a in c["at"]) == [0, 0, 2]
    clean, dirty = by["dirty/clean"], by["dirty/dirty"]
    assert np.array_equal(dirty["x"], clean["x"] | 0x80) and int(clean["x"].max()) == 1 and [call[0] for call in dirty["calls"]] == [0, 23, 24]
    assert [call[5].size for call in dirty["calls"]][:2] == [0, 0] and np.array_equal(dirty["calls"][2][5], clean["calls"][0][5])
    assert {124, 4114, 8024} <= set(clean["calls"][0][5].tolist())
    for P in (6, 64, 200):
        c = by["cuts/P%d" % P]
        cuts = [1, P - 1, P, P, P + 1, 1, 2 * P, 5000, 3, 8192, P]
        assert c["x"].size == 30000 and c["cuts"] == cuts + [30000 - sum(cuts)]
        d = M.distances_plain(c["preamble"], c["x"])
        assert all(d[a] == 0 for a in c["at"]) and len(c["at"]) == 6
        # calls that could do nothing still ask for the reserve; others leave exactly a preamble's length unconsumed
        assert [call[2] for call in c["calls"][:2]] == [0, 0] and all(call[3] == P + 1 for call in c["calls"])
        assert all(call[1] - call[2] == P for call in c["calls"][2:])
    assert len(cases) == 2 * len(GOLDEN_LENGTHS) + 18 + 32 + 2 + 3
