"""CPU tests of the exp, log, pow, root and trigonometric family: the fixture tests/golden/mathfn.npz against itself and against the
numpy model of the float32 rsqrt, the argument checks of the C ABI that return before a device is touched, the registry and the
descriptions of libpcx_math_blocks.so, the blocks' defaults, probes, signals and exceptions."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mathfn_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "math_blocks.cpp")
REF = "/root/reference"
GOLD = np.load(M.GOLD_PATH)
F64, F32, I32 = 0, 1, 3
PATHS = {"/comms/exp": 1, "/comms/exp2": 1, "/comms/exp10": 1, "/comms/expm1": 1, "/comms/expN": 2,
         "/comms/log": 1, "/comms/log2": 1, "/comms/log10": 1, "/comms/log1p": 1, "/comms/logN": 2, "/comms/pow": 2,
         "/comms/sqrt": 1, "/comms/cbrt": 1, "/comms/nth_root": 2, "/comms/rsqrt": 1, "/comms/sinc": 1, "/comms/sigmoid": 1, "/comms/trigonometric": 2}
REF_DOCS = {"exp": "Exp.cpp", "exp2": "Exp.cpp", "exp10": "Exp.cpp", "expm1": "Exp.cpp", "expN": "Exp.cpp", "log": "Log.cpp", "log2": "Log.cpp",
            "log10": "Log.cpp", "log1p": "Log.cpp", "logN": "Log.cpp", "pow": "Pow.cpp", "sqrt": "Root.cpp", "cbrt": "Root.cpp", "nth_root": "Root.cpp",
            "rsqrt": "RSqrt.cpp", "sinc": "Sinc.cpp", "sigmoid": "Sigmoid.cpp", "trigonometric": "Trigonometric.cpp"}


# ---------------------------------------------------------------- the fixture
def test_fixture_holds_every_case_and_its_own_distances():
    expected = set()
    for fn, p in M.CASES:
        for tname in M.TYPES:
            key = M.case_key(fn, p, tname)
            expected |= {key + "/ord", key + "/spec", key + "/e_ref"} | ({key + "/p"} if p is not None else set())
            x, ref, cr = GOLD[key + "/ord"]
            assert x.dtype == np.dtype(tname) and 190 <= x.size <= 210, key
            assert np.isfinite(x).all() and np.isfinite(ref).all() and np.isfinite(cr).all(), key
            d = M.ulp_distance(ref, cr)
            assert int(d.max()) == int(GOLD[key + "/e_ref"]) <= 4, (key, d.max())
            if p is not None:
                assert GOLD[key + "/p"].dtype == np.dtype(tname) and float(GOLD[key + "/p"]) == p, key
            sx, sref, scr = GOLD[key + "/spec"]
            settled = np.isfinite(sref) & (sref != 0)
            assert np.isnan(scr[~settled]).all(), key
            # (finite results of special inputs that have a truth lie as close to it as the ordinary ones)
            have = settled & np.isfinite(scr)
            assert M.ulp_distance(sref[have], scr[have]).max(initial=0) <= 4, key
    assert set(GOLD.files) == expected


def _has(values, wanted):
    bits = {v.tobytes() for v in values}
    return all(np.array(w, dtype=values.dtype).tobytes() in bits or (np.isnan(w) and np.isnan(values).any()) for w in wanted)


def test_fixture_special_groups():
    for fn, p in M.CASES:
        for tname in M.TYPES:
            key = M.case_key(fn, p, tname)
            sx, sref, _ = GOLD[key + "/spec"]
            fi = np.finfo(sx.dtype)
            # (the f(1 / x) operations on float32 keep the subnormals whose reciprocal is finite in float32: the fixture's script says why)
            inner_overflow = tname == "float32" and fn in ("ASEC", "ACSC", "ACOT", "ASECH", "ACSCH", "ACOTH")
            subnormals = [fi.tiny / 2] if inner_overflow else [fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2]
            assert _has(sx, [0.0, -0.0, np.inf, -np.inf, np.nan, fi.tiny, fi.max, -fi.max] + subnormals), key
            with np.errstate(all="ignore"):
                assert not inner_overflow or not (np.isinf(np.float32(1) / sx) & (sx != 0)).any(), key
    f32 = lambda fn: dict(zip(GOLD[fn + "/float32/spec"][0].tolist(), GOLD[fn + "/float32/spec"][1].tolist()))
    f64 = lambda fn: dict(zip(GOLD[fn + "/float64/spec"][0].tolist(), GOLD[fn + "/float64/spec"][1].tolist()))
    # the edges of the domains
    assert f64("LOG")[0.0] == -np.inf and np.isnan(f64("LOG")[-1.0]) and np.isnan(f32("LOG10")[-2.0]) and f32("LOG1P")[-1.0] == -np.inf
    assert np.isnan(f64("ACOS")[1.5]) and np.isnan(f32("ASIN")[-1.5]) and f64("ATANH")[1.0] == np.inf and f32("ATANH")[-1.0] == -np.inf
    assert f64("ACOSH")[1.0] == 0.0 and np.isnan(f32("ACOSH")[0.5]) and np.isnan(f64("SQRT")[-4.0])
    assert np.signbit(GOLD["SQRT/float32/spec"][1][list(GOLD["SQRT/float32/spec"][0]).index(0.0) + 1])         # sqrt(-0.0) is -0.0
    # overflow and underflow thresholds, on both sides
    for fn, (over32, under32, over64, under64) in {"EXP": ((88.5, 89.0), (-103.0, -104.5), (709.5, 710.0), (-745.0, -746.0)),
                                                    "EXP2": ((127.5, 128.0), (-149.0, -150.5), (1023.5, 1024.0), (-1074.0, -1075.5))}.items():
        for tab, over, under in ((f32(fn), over32, under32), (f64(fn), over64, under64)):
            assert np.isfinite(tab[over[0]]) and tab[over[1]] == np.inf and tab[under[0]] > 0 and tab[under[1]] == 0, fn
    assert np.isfinite(f32("SINH")[89.0]) and f32("SINH")[90.0] == np.inf and f32("SINH")[-90.0] == -np.inf
    assert np.isfinite(f64("SINH")[710.4]) and f64("SINH")[711.0] == np.inf
    # large trigonometric arguments
    for fn in ("COS", "SIN", "TAN", "SEC", "CSC", "COT"):
        for tname in M.TYPES:
            sx, sref, scr = GOLD["%s/%s/spec" % (fn, tname)]
            for big in (1e6, 1e22):
                at = list(sx).index(sx.dtype.type(big))
                assert np.isfinite(sref[at]) and np.isfinite(scr[at]), (fn, tname, big)
    # sinc on both sides of its threshold
    assert f64("SINC")[1e-7] == 1.0 and f64("SINC")[1.1e-6] < 1.0 and f32("SINC")[0.0] == 1.0
    # the float32 rsqrt on what a square root would refuse
    sx, sref, _ = GOLD["RSQRT/float32/spec"]
    assert (sx < 0).any() and (sx == 0).any() and np.isinf(sx).any() and ((sx != 0) & (np.abs(sx) < np.finfo(np.float32).tiny)).any()
    # what the expression the reference ends up in does with -0.0 and -inf (nth_root of 2 is pow, not sqrt)
    r2 = f64("NTH_ROOT@2")
    assert r2[-np.inf] == np.inf and r2[np.inf] == np.inf and np.isnan(r2[-4.0])
    sx, sref, _ = GOLD["NTH_ROOT@2/float64/spec"]
    assert not np.signbit(sref[1]) and sx[1] == 0 and np.signbit(sx[1])                 # pow(-0.0, 0.5) is +0.0
    assert f64("NTH_ROOT@3")[-27.0] == -3.0 and f32("NTH_ROOT@5")[-1.0] == -1.0 and np.isnan(f64("NTH_ROOT@-3")[-8.0]) and np.isnan(f64("NTH_ROOT@2.5")[-4.0])


def test_the_fixture_is_small():
    assert os.path.getsize(M.GOLD_PATH) < 512 * 1024


def test_rsqrt_model_equals_the_recorded_float32_rsqrt():
    for part in ("ord", "spec"):
        x, ref, _ = GOLD["RSQRT/float32/" + part]
        got = M.rsqrt_f32(x)
        keep = ~np.isnan(ref)
        assert keep.sum() >= 10 and np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(got[keep].view(np.uint32), ref[keep].view(np.uint32)), part
    # it is the approximation, not 1 / sqrt: about three digits
    x, ref, _ = GOLD["RSQRT/float32/ord"]
    rel = np.abs(ref.astype(np.float64) * np.sqrt(x.astype(np.float64)) - 1)
    assert 1e-5 < rel.max() < 1e-3


# ---------------------------------------------------------------- the C ABI's argument checks (none of these reaches a device)
def test_c_abi_refuses_what_it_cannot_run(pcx):
    L, lib = pcx._lib.load(), pcx._lib
    x = np.arange(64, dtype=np.float32)
    y = np.zeros(64, np.float32)
    px, py = x.ctypes.data, y.ctypes.data
    k = np.array([2.0], np.float32)
    k64 = np.array([2.0], np.float64)
    F = lib.MATH_FN

    def refused(rc, word):
        assert rc == lib.ERR_ARG and word in L.pcx_last_error().decode(), (rc, L.pcx_last_error())

    for sc in (I32, 2, 9, 10, -1):
        refused(L.pcx_mathfn(sc, F["EXP"], px, py, 8), "unsupported type")
        refused(L.pcx_mathfn_dev(sc, F["SQRT"], px, py, 8, None), "unsupported type")
        refused(L.pcx_mathfn_param(sc, F["POW"], k.ctypes.data, px, py, 8), "unsupported type")
        refused(L.pcx_mathfn_param_dev(sc, F["POW"], k.ctypes.data, px, py, 8, None), "unsupported type")
    for fn in (-1, 13, 15, 40, 47, 52, 1000):
        refused(L.pcx_mathfn(F32, fn, px, py, 8), "unknown function")
        refused(L.pcx_mathfn_param(F64, fn, k64.ctypes.data, px, py, 8), "unknown function")
    for name in lib.MATH_FN_PARAM:
        refused(L.pcx_mathfn(F32, F[name], px, py, 8), "takes a parameter")
        refused(L.pcx_mathfn_dev(F64, F[name], px, py, 8, None), "takes a parameter")
        refused(L.pcx_mathfn_param(F32, F[name], None, px, py, 8), "null parameter")
        refused(L.pcx_mathfn_param_dev(F32, F[name], None, px, py, 8, None), "null parameter")
    for name in M.PLAIN:
        refused(L.pcx_mathfn_param(F32, F[name], k.ctypes.data, px, py, 8), "takes no parameter")
    refused(L.pcx_mathfn_param_dev(F64, F["ACOTH"], k64.ctypes.data, px, py, 8, None), "takes no parameter")
    for base in (0.0, -0.0, -1.0, -np.inf):
        refused(L.pcx_mathfn_param(F32, F["LOGN"], np.array([base], np.float32).ctypes.data, px, py, 8), "Log base must be > 0")
        refused(L.pcx_mathfn_param_dev(F64, F["LOGN"], np.array([base], np.float64).ctypes.data, px, py, 8, None), "Log base must be > 0")
    # the overlap rule is checked before anything is queued
    refused(L.pcx_mathfn(F32, F["EXP"], px, px + 4, 8), "overlaps")
    refused(L.pcx_mathfn_dev(F64, F["LOG"], px + 8, px, 4, None), "overlaps")
    refused(L.pcx_mathfn_param(F32, F["POW"], k.ctypes.data, px, px + 16, 8), "overlaps")
    refused(L.pcx_mathfn(F32, F["EXP"], px, None, 8), "null buffer")
    assert np.array_equal(x, np.arange(64, dtype=np.float32)) and not y.any()
    # nothing to do: PCX_OK, whatever the pointers
    assert L.pcx_mathfn(F64, F["TAN"], None, None, 0) == lib.OK
    assert L.pcx_mathfn_param_dev(F32, F["NTH_ROOT"], k.ctypes.data, None, None, 0, None) == lib.OK
    assert set(F) == set(M.PLAIN) | set(M.PARAMS) and len(set(F.values())) == len(F) == 41


def test_python_wrapper_names_its_functions(dev, pcx):
    E = pcx._lib.InvalidArgument
    x = np.ones(4, np.float32)
    for call in (lambda: dev.math_fn("EXP3", x), lambda: dev.math_fn("POW", x), lambda: dev.math_fn("EXP", x, 2.0),
                 lambda: dev.math_fn("EXP", x.astype(np.int32)), lambda: dev.math_fn("LOGN", x, 0.0), lambda: dev.math_fn("SQRT", x, out=x[1:])):
        with pytest.raises(E):
            call()


# ---------------------------------------------------------------- the module
def make(path, *args, **kw):
    from pothoscomms_amd import blocks as B
    return B.make(path, *args, module="math", **kw)


def test_registry_has_the_eighteen_paths_with_their_arities():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("math") == sorted(PATHS)
    for path, arity in PATHS.items():
        assert B.registry_arity(path, module="math") == arity, path
    assert B.registry_arity("/comms/const_arithmetic", module="math") == -1 and B.registry_arity("/blocks/exp", module="math") == -1


EXT_PAIRS = {("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
SETTERS = {"/comms/expN": {("base", "setBase", "setter")}, "/comms/logN": {("base", "setBase", "setter")}, "/comms/pow": {("exponent", "setExponent", "setter")},
           "/comms/nth_root": {("root", "setRoot", "setter")}, "/comms/trigonometric": {("operation", "setOperation", "initializer")}}
MAKE_ARGS = {path: ("float32",) for path in ("/comms/exp", "/comms/exp2", "/comms/exp10", "/comms/expm1", "/comms/log", "/comms/log2", "/comms/log10", "/comms/log1p")}
MAKE_ARGS.update({path: ("float64",) for path in ("/comms/sqrt", "/comms/cbrt", "/comms/rsqrt", "/comms/sinc", "/comms/sigmoid")})
MAKE_ARGS.update({"/comms/expN": ("float32", 10.0), "/comms/logN": ("float32", 10.0), "/comms/pow": ("float64", 0.0), "/comms/nth_root": ("float64", 1.0),
                  "/comms/trigonometric": ("float32", "COS")})


def our_docs():
    return {d["factory"][0]: d for d in parse_docs(open(SRC).read())}


def test_descriptions_match_the_registry_and_the_registered_calls():
    docs = our_docs()
    assert set(docs) == set(PATHS)
    source_calls = registered_calls(open(SRC).read())
    for path, d in docs.items():
        assert len(d["factory"][1]) == PATHS[path], path
        # a block built from the description's own defaults
        defaults = [d["params"][k]["default"].strip('"') for k in d["factory"][1]]
        assert list(MAKE_ARGS[path]) == [type(a)(v) for a, v in zip(MAKE_ARGS[path], defaults)], path
        blk = make(path, *MAKE_ARGS[path])
        calls = blk.calls()
        pairs = set()
        for kind, fn, keys in d["calls"]:
            assert fn in source_calls and calls.get(fn) == 1 and len(keys) == 1, (path, fn)         # every setter: a registered call of one argument
            pairs.add((keys[0], fn, kind))
        assert pairs == SETTERS.get(path, set()) | EXT_PAIRS, path
        assert set(d["params"]) == {k for k, _, _ in pairs} | set(d["factory"][1]), path
        for key, p in d["params"].items():
            assert p["default"] is not None and " ".join(p["desc"]).strip(), (path, key)
            if p["options"]:
                assert p["default"] in p["options"], (path, key)
        assert " ".join(d["prose"]).strip() and d["category"] == ["/Math"]
        assert int(d["params"]["portSlabBytes"]["default"]) == blk.call("getPortSlabBytes") == 64 << 20
        blk.close()
    assert [o.strip('"') for o in docs["/comms/trigonometric"]["params"]["operation"]["options"]] == list(M.TRIG)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
@pytest.mark.parametrize("path", sorted(PATHS))
def test_descriptions_have_the_reference_schema_and_their_own_words(path):
    ours = our_docs()[path]
    ref = {d["factory"][0]: d for d in parse_docs(open(os.path.join(REF, "math", REF_DOCS[path.rsplit("/", 1)[1]])).read())}[path]
    assert ours["title"] == ref["title"] and ours["factory"] == ref["factory"] and ours["category"] == ref["category"]
    assert ours["alias"] == ref["alias"] == [] and ours["keywords"] == ref["keywords"]
    ext = {"device", "portSlabBytes"}
    assert [k for k in ours["order"] if k not in ext] == ref["order"] and set(ours["order"]) - set(ref["order"]) == ext
    assert {(fn, tuple(k), kind) for kind, fn, k in ours["calls"] if k[0] not in ext} == {(fn, tuple(k), kind) for kind, fn, k in ref["calls"]}
    for key, rp in ref["params"].items():
        for field in ("name", "default", "options", "widget", "preview", "tab", "units"):
            assert ours["params"][key][field] == rp[field], (key, field)

    def sentences(doc):
        text = " ".join(doc["prose"]) + " " + " ".join(" ".join(p["desc"]) for p in doc["params"].values())
        text = re.sub(r"<[^>]+>", " ", text)
        return {re.sub(r"\s+", " ", s).strip().lower() for s in re.split(r"[.;:]\s", text) if len(s.split()) >= 6}
    assert sentences(ours) and not (sentences(ours) & sentences(ref))


def test_block_defaults_ports_probes_and_exceptions(pcx):
    E = pcx._lib.InvalidArgument
    for path in PATHS:
        for dtype, size in (("float32", 4), ("float64", 8)):
            b = make(path, dtype, *MAKE_ARGS[path][1:], dimension=3)
            assert [p[1:4] for p in b.ports(0)] == [(dtype, 3, 3 * size)] == [p[1:4] for p in b.ports(1)], path
            assert set(b.calls()) >= {"setDevice", "getDevice", "setPortSlabBytes", "getPortSlabBytes"}
            b.close()
    for path, getter, setter in (("/comms/expN", "base", "setBase"), ("/comms/logN", "base", "setBase"), ("/comms/pow", "exponent", "setExponent"),
                                 ("/comms/nth_root", "root", "setRoot")):
        b = make(path, "float32", 0.1)
        assert b.call(getter) == float(np.float32(0.1))                  # converted to the element type
        assert b.calls()[getter] == 0 and b.calls()[setter] == 1 and b.calls()["probe" + getter.capitalize()] == 0
        for v in (2.0, 10.0, 3.0, 2.5):
            b.call(setter, v)
            assert b.call(getter) == v
        b = make(path, "float64", 0.1)
        assert b.call(getter) == 0.1
    # Log.cpp:188-191: a range error, at construction and afterwards; the base stays what it was
    b = make("/comms/logN", "float64", 3.0)
    for base in (0.0, -1.0):
        with pytest.raises(pcx._lib.PcxError, match="Log base must be > 0") as e:
            b.call("setBase", base)
        assert not isinstance(e.value, E)
        with pytest.raises(pcx._lib.PcxError, match="Log base must be > 0"):
            make("/comms/logN", "float32", base)
    assert b.call("base") == 3.0
    make("/comms/expN", "float32", -1.0).close()          # (no such check on the exponential's base)
    # Trigonometric.cpp:510: an invalid argument, at construction and afterwards
    b = make("/comms/trigonometric", "float64", "ACOTH")
    assert "setOperation" in b.calls()
    for op in ("cos", "ARCSIN", ""):
        with pytest.raises(E, match="Invalid operation"):
            b.call("setOperation", op)
        with pytest.raises(E, match="Invalid operation"):
            make("/comms/trigonometric", "float32", op)
    for op in M.TRIG:
        b.call("setOperation", op)
    # an integer or complex dtype, with the words the reference's factories use for a type they do not know
    for path in PATHS:
        words = "Unsupported dtype" if path == "/comms/rsqrt" else "unsupported type"
        for dtype in ("int32", "uint8", "int64", "complex_float32"):
            with pytest.raises(E, match=words):
                make(path, dtype, *MAKE_ARGS[path][1:])


def test_signals_reach_a_connected_slot():
    """setBase / setExponent / setRoot emit their signal without a value (Exp.cpp:180, Log.cpp:200, Pow.cpp:102, Root.cpp:251): a slot of
    one argument refuses it, after the setter took effect; the probes fire <name>Triggered"""
    for path, getter, setter in (("/comms/expN", "base", "setBase"), ("/comms/logN", "base", "setBase"), ("/comms/pow", "exponent", "setExponent"),
                                 ("/comms/nth_root", "root", "setRoot")):
        src, sink = make(path, "float64", 2.0), make("/comms/pow", "float64", 0.0)
        src.connect_signal(getter + "Changed", sink, "setExponent")
        with pytest.raises(Exception, match="wrong number of arguments"):
            src.call(setter, 7.0)
        assert src.call(getter) == 7.0 and sink.call("exponent") == 0.0
        src.connect_signal(getter + "Triggered", sink, "setExponent")
        with pytest.raises(Exception, match="no such signal"):
            src.connect_signal("operationChanged", sink, "setExponent")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_source_type_checks_against_the_pothos_surface():
    blocks = os.path.dirname(SRC)
    flags = ["-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-DPCX_WITH_POTHOS",
             "-I" + os.path.join(ROOT, "tests", "pothos_decl"), "-I" + os.path.join(ROOT, "include"), "-I" + blocks]
    r = subprocess.run(["g++"] + flags + [SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_port_slab_default_is_the_one_of_the_other_modules():
    pat = r"constexpr size_t kPortSlabBytes = (\d+)u << (\d+);"
    a = re.search(pat, open(os.path.join(os.path.dirname(SRC), "comms_blocks.cpp")).read())
    b = re.search(pat, open(SRC).read())
    assert a and b and int(a.group(1)) << int(a.group(2)) == int(b.group(1)) << int(b.group(2))


def test_the_module_library_exports_the_runner_and_nothing_of_the_blocks():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_math_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"pcxb_make_args", "pcxb_work", "pcxb_work_ports", "pcxb_call_double", "pcxb_get_double", "pcxb_registry_path"} <= exported
    assert all(s.startswith("pcxb_") for s in exported), sorted(s for s in exported if not s.startswith("pcxb_"))
