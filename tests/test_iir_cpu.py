"""CPU suite of /comms/iir_filter: the sequential model (tests/iir_model.py) against closed forms and scipy, its designer, the plan and
bound restated, the residual check, the C ABI's argument checks, the registry of libpcx_iir_blocks.so and the block's description."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import iir_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "iir_blocks.cpp")
REF = "/root/reference"


def test_first_order_impulse_response_is_exactly_half_to_the_n():
    x = np.zeros(200)
    x[0] = 1.0
    yd, _ = M.run(x, [1.0, 0.0, 1.0, -0.5], "float64")
    assert np.array_equal(yd, 0.5 ** np.arange(200))


def test_default_taps_dc_gain():
    b, a = M.normalise(M.DEFAULT_TAPS)
    yd, _ = M.run(np.ones(5000), M.DEFAULT_TAPS, "float64")
    assert abs(yd[-1] - b.sum() / a.sum()) < 1e-12


def test_model_carries_its_history_across_calls():
    x = np.random.default_rng(1).uniform(-1, 1, (3000, 2))
    taps = M.named_set()["butter4_0.1"]
    whole = M.Model(taps, True).process_double(x)
    m = M.Model(taps, True)
    parts = np.concatenate([m.process_double(x[a:b]) for a, b in ((0, 1), (1, 38), (38, 1000), (1000, 3000))])
    assert np.array_equal(whole, parts)


def test_model_against_scipy_lfilter_over_the_named_set():
    ss = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(2).uniform(-1, 1, 4000)
    for name, taps in M.named_set().items():
        plan, bound = M.plan(taps)
        b, a = M.normalise(taps)
        yd, _ = M.run(x, taps, "float64")
        ref = ss.lfilter(b, a, x)
        assert plan == "SCAN" and np.max(np.abs(yd - ref)) <= bound * np.max(np.abs(x)), name


def test_designer_against_scipy():
    ss = pytest.importorskip("scipy.signal")
    for order, wn in ((2, 0.02), (2, 0.2), (4, 0.2), (6, 0.4), (8, 0.1)):
        b, a = M.butter(order, wn)
        rb, ra = ss.butter(order, wn)
        assert np.allclose(b, rb, rtol=1e-12, atol=1e-15) and np.allclose(a, ra, rtol=1e-12, atol=1e-15), (order, wn)
    b, a = M.cheby1(4, 0.1, 0.4)
    rb, ra = ss.cheby1(4, 0.1, 0.4)
    assert np.allclose(b, rb, rtol=1e-12, atol=1e-15) and np.allclose(a, ra, rtol=1e-12, atol=1e-15)
    # the reference's default taps are butter(2, 0.2) to three digits
    assert np.allclose(M.taps_of(M.butter(2, 0.2)), M.DEFAULT_TAPS, atol=1e-3)


def test_named_set_plans_scan_within_1e_10_and_unstable_filters_serial():
    for name, taps in M.named_set().items():
        plan, bound = M.plan(taps)
        assert plan == "SCAN" and 0 < bound <= 1e-10, (name, plan, bound)
    for taps in ([1, 0, 1, -1.01], [1, 0, 1, -1], [1, 0, 0, 1, 0, 1]):
        assert M.plan(taps) == ("SERIAL", 0.0), taps
    assert M.schur_cohn([1, -0.5]) == [-0.5]
    assert M.plan([2, 1])[0] == "SCAN"


def test_high_order_set_meets_the_conditions_its_gpu_tests_rest_on():
    """what keeps a tolerance of the GPU tests from hiding a fault: a bound below 1e-10 on every SCAN filter, no feedforward tap
    below 0.01 (of an l1 norm of 1), no feedback tap of a spread filter below 1e-5 (dropping any one tap moves a float64 output by
    far more than bound * max|x|), all the feedback of a comb on its oldest slot; the unstable filters SERIAL and within 1e7 over
    the 3000 samples they are run on, so that every output and every slot of the history still counts in double"""
    hs = M.high_order_set()
    assert sorted(hs) == sorted(["spread%d" % n for n in (9, 12, 16, 17, 24, 31, 32)] + ["comb%d" % n for n in (9, 16, 17, 31, 32)]
                                + ["unstable%d" % n for n in (3, 9, 16, 17, 31, 32)])
    x = np.random.default_rng(7).uniform(-1, 1, 3000)
    for name, taps in hs.items():
        N = int(re.search(r"\d+$", name).group())
        b, a = M.normalise(taps)
        assert len(taps) == 2 * (N + 1) and a[0] == 1.0, name
        assert np.min(np.abs(b)) >= 0.01 and abs(np.abs(b).sum() - 1) < 1e-12, (name, np.min(np.abs(b)))
        plan, bound = M.plan(taps)
        if name.startswith("unstable"):
            assert (plan, bound) == ("SERIAL", 0.0), name
            yd, _ = M.run(x, taps, "float64")
            assert np.all(np.isfinite(yd)) and 1e3 < np.max(np.abs(yd)) < 1e7, (name, np.max(np.abs(yd)))
            continue
        assert plan == "SCAN" and 0 < bound <= 1e-10, (name, plan, bound)
        if name.startswith("spread"):
            assert np.min(np.abs(a)) >= 1e-5, (name, np.min(np.abs(a)))
        else:
            assert np.count_nonzero(a) == 2 and abs(a[N]) >= 0.5, name


def test_high_order_model_against_scipy_and_across_short_calls():
    ss = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(8).uniform(-1, 1, (600, 2))
    cuts = [1, 1, 2, 5, 16, 7, 31, 32, 33, 64, 408]
    for name, taps in M.high_order_set().items():
        if name.startswith("unstable"):
            continue
        b, a = M.normalise(taps)
        whole = M.Model(taps, True).process_double(x)
        assert np.max(np.abs(whole - ss.lfilter(b, a, x, axis=0))) <= M.plan(taps)[1], name
        m, pos, parts = M.Model(taps, True), 0, []
        for c in cuts:
            parts.append(m.process_double(x[pos:pos + c]))
            pos += c
        assert pos == 600 and np.array_equal(whole, np.concatenate(parts)), name


def test_narrowing():
    y = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 127.9, -128.9, 3.7, -3.7, -0.2])
    assert M.narrow(y, "int8").tolist() == [0, 127, -128, 127, -128, 127, -128, 3, -3, 0]
    assert M.narrow(np.array([2.0 ** 63, -2.0 ** 63, 2.0 ** 62 + 0.5]), "int64").tolist() == [2 ** 63 - 1, -2 ** 63, 2 ** 62]
    assert M.narrow(np.array([1.0 + 2.0 ** -30]), "float32")[0] == np.float32(1.0)


def test_residual_check_finds_ulp_changes_and_no_false_alarm():
    """the tolerance of a sample holds the narrowing of its N neighbours, as large as one ulp of its own: a single-ulp change is
    found where the neighbours' rounding leaves room, a few ulps nearly everywhere (the short streams compare with the model itself)"""
    x = np.random.default_rng(3).uniform(-1, 1, 3000)
    taps = M.named_set()["default"]
    plan, bound = M.plan(taps)
    for name in ("float32", "float64"):
        _, y = M.run(x, taps, name)
        assert M.residual_check(x, y.astype(np.float64), taps, name, 0.0) == -1, name
    yd, y = M.run(x, taps, "float32")
    found = {1: 0, 4: 0}
    for ulps in found:
        for i in range(100, 3000, 29):
            bad = y.copy()
            away = np.float32(np.inf) if yd[i] <= y[i] else np.float32(-np.inf)
            for _ in range(ulps):
                bad[i] = np.nextafter(bad[i], away)
            found[ulps] += i <= M.residual_check(x, bad.astype(np.float64), taps, "float32", 0.0) <= i + 2
    assert found[1] >= 30 and found[4] >= 90, found
    _, y = M.run(x * 1000, taps, "int16")
    assert M.residual_check(x * 1000, y.astype(np.float64), taps, "int16", bound) == -1
    bad = y.copy()
    bad[777] += 3
    assert M.residual_check(x * 1000, bad.astype(np.float64), taps, "int16", bound) in (777, 778, 779)


# ---- the C ABI (no device is touched: the taps are checked before the handle)
@pytest.mark.parametrize("taps, why", [([], "Order cannot 0"), ([1.0, 2.0, 3.0], "same length"), ([0.5] * 68, "at most 66"),
                                       ([1.0, 0.0], "a[0] is 0"), ([1.0, 0.2, 1.0, float("nan")], "not finite")])
def test_abi_refuses_bad_taps_before_touching_the_device(pcx, taps, why):
    L = pcx._lib.load()
    t = (C.c_double * max(1, len(taps)))(*taps)
    assert L.pcx_iir_set_taps(None, t, len(taps)) == pcx._lib.ERR_ARG
    assert why in pcx._lib.last_error(), pcx._lib.last_error()


def test_abi_refuses_bad_handles_and_types(pcx):
    L = pcx._lib.load()
    h = C.c_void_p()
    assert L.pcx_iir_create(7, 0, C.byref(h)) == pcx._lib.ERR_ARG
    assert L.pcx_iir_create(-1, 1, C.byref(h)) == pcx._lib.ERR_ARG
    t = (C.c_double * 4)(1.0, 0.0, 1.0, -0.5)
    assert L.pcx_iir_set_taps(None, t, 4) == pcx._lib.ERR_ARG and "null handle" in pcx._lib.last_error()
    assert L.pcx_iir_process(None, None, None, 1) == pcx._lib.ERR_ARG
    assert L.pcx_iir_process_dev(None, None, None, 1, None) == pcx._lib.ERR_ARG
    p, b = C.c_int(), C.c_double()
    assert L.pcx_iir_get_plan(None, C.byref(p), C.byref(b)) == pcx._lib.ERR_ARG


# ---- the block (libpcx_iir_blocks.so)
def test_module_registry_holds_the_iir_filter_and_its_alias():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("iir") == ["/blocks/iir_filter", "/comms/iir_filter"]
    for path in ("/comms/iir_filter", "/blocks/iir_filter"):
        assert B.registry_arity(path, module="iir") == 1
        assert path not in B.registry_paths()
        for other in ("filter", "envelope"):
            assert path not in B.module_registry_paths(other)


def test_factory_rejects_unsupported_types():
    from pothoscomms_amd import _lib, blocks as B
    for dtype, dim in (("uint8", 1), ("complex_uint16", 1), ("float32", 2), ("complex_int16", 4)):
        with pytest.raises(_lib.InvalidArgument, match="unsupported type"):
            B.make("/comms/iir_filter", dtype, module="iir", dimension=dim)


def test_description_matches_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert len(docs) == 1
    d = docs[0]
    assert d["factory"] == ("/comms/iir_filter", ["dtype"])
    calls = registered_calls(text)
    pairs = set()
    for kind, fn, keys in d["calls"]:
        assert fn in calls and len(keys) == 1, fn
        pairs.add((keys[0], fn, kind))
    assert pairs == {("taps", "setTaps", "setter"), ("waitTaps", "setWaitTaps", "setter"),
                     ("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
    assert d["params"]["taps"]["default"] == "[0.0676, 0.135, 0.0676, 1, -1.142, 0.412]"
    assert d["params"]["waitTaps"]["default"] == "false"
    assert calls >= {"getTaps", "getWaitTaps", "getDevice", "getPortSlabBytes"}
    assert "|alias /blocks/iir_filter" in text and "|category /Filter" in text


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_description_has_the_reference_schema_and_its_own_words():
    import re
    ours = parse_docs(open(SRC).read())[0]
    ref = parse_docs(open(os.path.join(REF, "filter", "IIRFilter.cpp")).read())[0]
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
