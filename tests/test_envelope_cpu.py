"""CPU suite of /comms/envelope_detector: the numpy restatement (tests/envelope_model.py) against the reference's recorded outputs,
the registry of libpcx_envelope_blocks.so, the block's description, and the Pothos branch of its source."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import envelope_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "envelope.npz")
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "envelope_blocks.cpp")
REF = "/root/reference"
DTYPES = [t for t in M.SCALARS] + ["complex_" + t for t in M.SCALARS]
TIMES = {"10_10": (10.0, 10.0), "1_50": (1.0, 50.0), "0_10": (0.0, 10.0), "1000_3": (1000.0, 3.0), "unset": None}


def golden_cases():
    z = np.load(GOLDEN)
    for k in z.files:
        if k.startswith("out/"):
            _, dtype, pattern, tk, L = k.split("/")
            yield dtype, pattern, TIMES[tk], int(L), z["in/%s/%s" % (dtype, pattern)], z[k]


def gains_of(times):
    return M.gains(*times) if times is not None else M.gains()


def test_fixture_covers_every_type_time_and_lookahead():
    seen = set()
    for dtype, pattern, times, L, x, ref in golden_cases():
        seen.add((dtype, times, L))
        assert ref.dtype == np.float32 and ref.shape[0] == x.shape[0] - L
    assert len(seen) == 12 * 5 * 2
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_restatement_equals_the_reference_outputs():
    n = 0
    for dtype, pattern, times, L, x, ref in golden_cases():
        got, _ = M.run(M.magnitude(x, dtype)[L:], gains_of(times))
        assert M.same(got, ref), (dtype, pattern, times, L)
        n += 1
    assert n == 560


def test_the_issue_magnitudes():
    cases = [("complex_int16", (3, 4), 4), ("complex_int16", (5, 5), 7), ("complex_int16", (-7, 7), 9),
             ("complex_int16", (-32768, 5), -32768), ("complex_int8", (-128, 1), -128), ("complex_int32", (-2 ** 31, 1), 1)]
    for dtype, v, want in cases:
        x = np.array([v], dtype=M.SCALARS[M.split(dtype)[0]])
        assert M.magnitude(x, dtype)[0] == want, (dtype, v)
    assert M.magnitude(np.array([-2 ** 31], np.int32), "int32")[0] == -2147483648.0
    assert M.magnitude(np.array([-128], np.int8), "int8")[0] == 128.0


def test_check_steps_finds_a_broken_output():
    x = np.random.default_rng(1).uniform(-1, 1, (5000, 2)).astype(np.float32)
    g = M.gains(10.0, 30.0)
    mag = M.magnitude(x, "complex_float32")
    out, _ = M.run(mag, g, 0.25)
    assert M.check_steps(mag, out, 0.25, g) == -1
    bad = out.copy()
    bad[1234] = np.nextafter(bad[1234], np.float32(2))
    assert M.check_steps(mag, bad, 0.25, g) == 1234


# ---- the block (libpcx_envelope_blocks.so)
def test_module_registry_holds_the_envelope_detector_and_its_alias():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("envelope") == ["/blocks/envelope_detector", "/comms/envelope_detector"]
    for path in ("/comms/envelope_detector", "/blocks/envelope_detector"):
        assert B.registry_arity(path, module="envelope") == 1
        assert path not in B.registry_paths()
    assert "/comms/envelope_detector" not in B.module_registry_paths("filter")


def test_factory_rejects_unsupported_types():
    from pothoscomms_amd import _lib, blocks as B
    for dtype, dim in (("uint8", 1), ("complex_uint16", 1), ("float32", 2), ("complex_int16", 4)):
        with pytest.raises(_lib.InvalidArgument, match="unsupported type"):
            B.make("/comms/envelope_detector", dtype, module="envelope", dimension=dim)


def test_abi_refuses_bad_arguments_before_touching_the_device(pcx):
    import ctypes as C
    L = pcx._lib.load()
    h = C.c_void_p()
    assert L.pcx_envelope_create(7, 0, C.byref(h)) == pcx._lib.ERR_ARG
    assert L.pcx_envelope_set_attack(None, 1.0) == pcx._lib.ERR_ARG
    assert L.pcx_envelope_process(None, None, None, 1) == pcx._lib.ERR_ARG


def test_description_matches_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert len(docs) == 1
    d = docs[0]
    assert d["factory"] == ("/comms/envelope_detector", ["dtype"])
    calls = registered_calls(text)
    pairs = set()
    for kind, fn, keys in d["calls"]:
        assert fn in calls and len(keys) == 1, fn
        pairs.add((keys[0], fn, kind))
    assert pairs == {("attack", "setAttack", "setter"), ("release", "setRelease", "setter"), ("lookahead", "setLookahead", "setter"),
                     ("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
    for key in ("attack", "release", "lookahead"):
        assert d["params"][key]["default"] == "10" and d["params"][key]["units"] == "samples"
    assert calls >= {"getAttack", "getRelease", "getLookahead", "getDevice", "getPortSlabBytes"}
    assert "|alias /blocks/envelope_detector" in text


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_description_has_the_reference_schema_and_its_own_words():
    import re
    ours = parse_docs(open(SRC).read())[0]
    ref = parse_docs(open(os.path.join(REF, "filter", "EnvelopeDetector.cpp")).read())[0]
    assert ours["title"] == ref["title"] and ours["factory"] == ref["factory"] and ours["category"] == ref["category"]
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
    assert int(parse_docs(open(SRC).read())[0]["params"]["portSlabBytes"]["default"]) == int(a.group(1)) << int(a.group(2))
