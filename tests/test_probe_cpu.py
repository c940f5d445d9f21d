"""CPU suite of /comms/signal_probe: the registry of libpcx_probe_blocks.so, the pcx_probe_* family of the C ABI and its argument
checks, the Python handle, the block's defaults, calls and description, and the soundness of what the GPU suite stands on: on every
input of tests/test_probe_gpu.py the sequential model (tests/probe_model.py) lies within its bound of the exact truth.  No device is
touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import probe_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "probe_blocks.cpp")
REF = "/root/reference"
PATHS = ["/blocks/stream_probe", "/comms/signal_probe"]
# (probeValue is the slot registerProbe("value") adds)
CALLS = {"value": 0, "setMode": 1, "getMode": 0, "setWindow": 1, "getWindow": 0, "setRate": 1, "getRate": 0, "setDevice": 1, "getDevice": 0,
         "setPortSlabBytes": 1, "getPortSlabBytes": 0, "probeValue": 0}
FAMILY = ["create", "destroy", "set_mode", "get_mode", "set_window", "get_window", "get_geometry", "process", "process_dev", "windows", "windows_dev"]
OTHER_MODULES = ("filter", "envelope", "iir", "digital", "correlator", "symbol", "repack", "waveform", "utility", "framer", "logic", "math", "special")


def make(path, dtype, **kw):
    from pothoscomms_amd import blocks as B
    return B.make(path, dtype, module="probe", **kw)


# ---- the registry and the C ABI
def test_module_registry_holds_the_two_paths_with_arity_1():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("probe") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="probe") == 1
        assert path not in B.registry_paths()
        for other in OTHER_MODULES:
            assert path not in B.module_registry_paths(other), other
    assert B.module_registry_paths("utility") == ["/blocks/threshold", "/comms/threshold"]


def test_header_declares_the_family_and_the_binding_covers_it(pcx):
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    family = sorted(set(re.findall(r"PCX_API\s+int\s+(pcx_probe_\w+)\s*\(", src)))
    assert family == sorted("pcx_probe_" + n for n in FAMILY)
    assert sorted(n for n in pcx._lib.SIGNATURES if n.startswith("pcx_probe_")) == family
    out = subprocess.run(["nm", "-D", "--defined-only", pcx._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(family) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert re.search(r"enum\s*\{\s*PCX_PROBE_VALUE = 0, PCX_PROBE_RMS = 1, PCX_PROBE_MEAN = 2\s*\}", src)
    assert (pcx._lib.PROBE_VALUE, pcx._lib.PROBE_RMS, pcx._lib.PROBE_MEAN) == (0, 1, 2)


def test_abi_argument_errors_come_before_any_device_call(pcx):
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    buf = (C.c_double * 8)()
    h, n, mode, a, b, c = C.c_void_p(), C.c_size_t(7), C.c_int(7), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.pcx_probe_create(None, pcx._lib.F32, 1) == E
    for bad in (pcx._lib.U64, pcx._lib.U32, pcx._lib.U16, pcx._lib.U8, -1, 10):
        for cplx in (0, 1):
            assert L.pcx_probe_create(C.byref(h), bad, cplx) == E and "unsupported type" in pcx._lib.last_error() and not h.value
    assert L.pcx_probe_set_mode(None, 0) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_probe_set_window(None, 4) == E and L.pcx_probe_get_window(None, C.byref(n)) == E and L.pcx_probe_get_mode(None, C.byref(mode)) == E
    assert L.pcx_probe_process(None, buf, 4, buf, C.byref(n)) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_probe_process_dev(None, buf, 4, buf, C.byref(n), None) == E
    assert L.pcx_probe_windows(None, buf, 4, buf) == E and L.pcx_probe_windows_dev(None, buf, 4, buf, None) == E
    assert L.pcx_probe_get_geometry(None, C.byref(a), C.byref(b), C.byref(c)) == E
    for scalar in (pcx._lib.F64, pcx._lib.F32, pcx._lib.I64, pcx._lib.I32, pcx._lib.I16, pcx._lib.I8):
        for cplx in (0, 1):
            assert L.pcx_probe_create(C.byref(h), scalar, cplx) == 0
            try:
                # the constructor's values (SignalProbe.cpp:64-67)
                assert L.pcx_probe_get_mode(h, C.byref(mode)) == 0 and mode.value == pcx._lib.PROBE_VALUE
                assert L.pcx_probe_get_window(h, C.byref(n)) == 0 and n.value == 1024
                assert L.pcx_probe_set_mode(h, 3) == E and L.pcx_probe_set_mode(h, -1) == E and "unknown mode" in pcx._lib.last_error()
                assert L.pcx_probe_set_window(h, 0) == E and "window" in pcx._lib.last_error()
                assert L.pcx_probe_get_window(h, C.byref(n)) == 0 and n.value == 1024
                assert L.pcx_probe_set_mode(h, pcx._lib.PROBE_MEAN) == 0 and L.pcx_probe_get_mode(h, C.byref(mode)) == 0 and mode.value == 2
                # geometry in elements of the type: whole 16-byte units, the large-window path right behind the tile
                es = {pcx._lib.F64: 8, pcx._lib.F32: 4, pcx._lib.I64: 8, pcx._lib.I32: 4, pcx._lib.I16: 2, pcx._lib.I8: 1}[scalar] * (2 if cplx else 1)
                assert L.pcx_probe_get_geometry(h, C.byref(a), None, C.byref(c)) == E
                assert L.pcx_probe_get_geometry(h, C.byref(a), C.byref(b), C.byref(c)) == 0
                assert a.value * es % (256 * 16) == 0 and b.value * es % (256 * 16) == 0 and c.value == a.value + 1 and b.value <= a.value
                # null counts, values and buffers
                assert L.pcx_probe_process(h, buf, 4, buf, None) == E and "null count" in pcx._lib.last_error()
                assert L.pcx_probe_process(h, buf, 4, None, C.byref(n)) == E and "null value" in pcx._lib.last_error()
                assert L.pcx_probe_process(h, None, 4, buf, C.byref(n)) == E and "null buffer" in pcx._lib.last_error()
                assert L.pcx_probe_process_dev(h, buf, 4, buf, None, None) == E and L.pcx_probe_process_dev(h, None, 4, buf, C.byref(n), None) == E
                assert L.pcx_probe_windows(h, None, 4, buf) == E and L.pcx_probe_windows(h, buf, 4, None) == E
                assert L.pcx_probe_windows_dev(h, None, 4, buf, None) == E and L.pcx_probe_windows_dev(h, buf, 4, None, None) == E
                # no element: nothing consumed, the value untouched, no device call
                buf[0], buf[1] = 3.5, -2.25
                n.value = 7
                assert L.pcx_probe_process(h, None, 0, buf, C.byref(n)) == 0 and n.value == 0 and (buf[0], buf[1]) == (3.5, -2.25)
                n.value = 7
                assert L.pcx_probe_process_dev(h, None, 0, buf, C.byref(n), None) == 0 and n.value == 0 and (buf[0], buf[1]) == (3.5, -2.25)
                assert L.pcx_probe_windows(h, None, 0, None) == 0 and L.pcx_probe_windows_dev(h, None, 0, None, None) == 0
            finally:
                assert L.pcx_probe_destroy(h) == 0
                h = C.c_void_p()


def test_the_python_handle(dev):
    p = dev.SignalProbe()
    assert (p.dtype, p.mode, p.window) == ("complex_float32", "VALUE", 1024)
    tile, slc, switch = p.geometry()
    assert tile * 8 % 4096 == 0 and switch == tile + 1 and slc <= tile
    assert p.process(np.zeros((0, 2), np.float32)) == (None, 0)
    assert p.windows(np.zeros(0, np.complex64)).shape == (0,)
    p.set_mode("RMS")
    p.set_window(77)
    assert (p.mode, p.window) == ("RMS", 77)
    with pytest.raises(ValueError):
        p.set_mode("PEAK")
    with pytest.raises(ValueError):
        p.set_window(0)
    with pytest.raises(ValueError):
        p.process(np.zeros(4, np.float32))             # a real array for a complex probe
    p.close()
    for dtype in M.TYPES:
        q = dev.SignalProbe(dtype, "MEAN", 3)
        assert q.is_complex == M.is_complex(dtype) and q.np_dtype == M.scalar_of(dtype) and q.window == 3
        q.close()
    for bad in ("uint8", "uint16", "complex_uint32", "uint64"):
        with pytest.raises(ValueError, match="unsupported type"):
            dev.SignalProbe(bad)


# ---- the block (libpcx_probe_blocks.so)
@pytest.mark.parametrize("dtype", M.TYPES)
def test_a_fresh_block_answers_the_constructors_values(dtype):
    for path in PATHS:
        b = make(path, dtype)
        assert (b.in_dtype, b.in_dim, b.out_dtype, b.out_dim) == (dtype, 1, None, 0)
        assert [p[:3] for p in b.ports(0)] == [("0", dtype, 1)] and b.ports(1) == []
        assert (b.call("getMode"), b.call("getWindow"), b.call("getRate")) == ("VALUE", 1024, 0.0)
        v = b.call("value")
        assert v == 0 and type(v) is (complex if M.is_complex(dtype) else float)
        assert b.calls() == CALLS
        assert b.initial_reserve() == 1 and b.reserve() == 1                   # SignalProbe.cpp:79
        b.call("setWindow", 4097)
        assert b.call("getWindow") == 4097 and b.reserve() == 4097             # :100
        with pytest.raises(ValueError, match="window cannot be 0"):
            b.call("setWindow", 0)
        assert b.call("getWindow") == 4097 and b.reserve() == 4097
        b.call("setRate", 2.5)
        assert b.call("getRate") == 2.5
        for mode in ("RMS", "MEAN", "VALUE", "PEAK", ""):                      # any string is kept (:87-90)
            b.call("setMode", mode)
            assert b.call("getMode") == mode
        # no elements: nothing is consumed
        x = np.zeros((0, 2) if M.is_complex(dtype) else 0, M.scalar_of(dtype))
        outs, consumed, produced = b.work_ports([x], [])
        assert (outs, consumed, produced) == ([], [0], []) and b.call("value") == 0
        b.close()


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "uint32", "uint64", "complex_uint8", "complex_uint32"])
def test_an_unsupported_type_throws(dtype):
    for path in PATHS:
        with pytest.raises(ValueError, match="unsupported type"):
            make(path, dtype)


def test_a_vector_stream_throws():
    for dtype in ("float32", "complex_int16"):
        with pytest.raises(ValueError, match="unsupported type"):
            make(PATHS[1], dtype, dimension=2)


def test_signals_and_slots_are_registered():
    a, b = make(PATHS[1], "float32"), make(PATHS[1], "float64")
    a.connect_signal("valueChanged", b, "setRate")
    a.connect_signal("valueTriggered", b, "setRate")
    with pytest.raises(Exception):
        a.connect_signal("valueDropped", b, "setRate")
    b.call("setRate", 9.0)
    a.call("probeValue")                           # emits valueTriggered with value() = 0
    assert b.call("getRate") == 0.0
    a.close()
    b.close()


def test_description_matches_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert [d["factory"] for d in docs] == [("/comms/signal_probe", ["dtype"])]
    calls = registered_calls(text)
    assert calls == set(CALLS) - {"probeValue"}
    assert re.search(r'registerProbe\("value"\)', text) and re.search(r'registerSignal\("valueChanged"\)', text)
    d = docs[0]
    pairs = set()
    for kind, fn, keys in d["calls"]:
        assert fn in calls and len(keys) == 1, fn
        pairs.add((keys[0], fn, kind))
    assert pairs == {("mode", "setMode", "setter"), ("rate", "setRate", "setter"), ("window", "setWindow", "setter"),
                     ("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
    assert set(d["params"]) == {k for k, _, _ in pairs} | {"dtype"}
    assert d["order"] == ["dtype", "mode", "rate", "window", "device", "portSlabBytes"]
    assert d["params"]["dtype"]["default"] == '"complex_float32"' and d["params"]["window"]["default"] == "1024"
    assert d["params"]["mode"]["options"] == ['"VALUE"', '"RMS"', '"MEAN"'] and d["params"]["mode"]["default"] == '"VALUE"'
    assert d["alias"] == ["/blocks/stream_probe"] and d["category"] == ["/Utility", "/Event"]
    for p in d["params"].values():
        assert " ".join(p["desc"]).strip() and p["default"] is not None
    assert " ".join(d["prose"]).strip()


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_description_has_the_reference_schema_and_its_own_words():
    ours = parse_docs(open(SRC).read())[0]
    ref = parse_docs(open(os.path.join(REF, "utility", "SignalProbe.cpp")).read())[0]
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
    blk = make(PATHS[1], "int16")
    assert blk.call("getPortSlabBytes") == int(a.group(1)) << int(a.group(2))
    blk.close()


def test_the_module_library_exports_the_runner_and_nothing_of_the_block():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_probe_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"pcxb_make", "pcxb_work_ports", "pcxb_activate", "pcxb_call_double", "pcxb_get_double", "pcxb_get_complex", "pcxb_call_string",
            "pcxb_get_string", "pcxb_call_void", "pcxb_input_reserve", "pcxb_connect_signal", "pcxb_registry_path"} <= exported
    assert all(s.startswith("pcxb_") for s in exported), sorted(s for s in exported if not s.startswith("pcxb_"))


def test_the_build_lists_the_module_and_the_kernels():
    mk = open(os.path.join(ROOT, "pothoscomms_amd", "csrc", "Makefile")).read()
    assert " probe.hip" in mk and " pcx_prb_api.hip" in mk and re.search(r"^MODULES\s*:=.*\bprobe\b", mk, flags=re.M)
    from pothoscomms_amd import blocks as B
    assert B.MODULES["probe"].endswith("libpcx_probe_blocks.so")


# ---- what the GPU suite stands on
def geometry_of(dev):
    cache = {}

    def g(dtype):
        if dtype not in cache:
            p = dev.SignalProbe(dtype)
            cache[dtype] = p.geometry()
            p.close()
        return cache[dtype]
    return g


def test_the_model_restates_the_loop():
    """the vectorised model against the plain loop of SignalProbe.cpp:141-160 written out, on short windows of every type"""
    for dtype in M.TYPES:
        for n in (1, 2, 3, 65):
            x = M.make_input(dtype, n)
            z = M.to_double(x)
            acc, mre, mim = 0.0, 0.0, 0.0
            for v in z:
                a = float(np.abs(np.complex128(v)))
                acc += a * a
                mre += float(np.real(v))
                mim += float(np.imag(v))
            assert M.model(x, "RMS") == (float(np.sqrt(np.float64(acc) / n)), 0.0), (dtype, n)
            assert M.model(x, "MEAN") == (mre / n, mim / n if M.is_complex(dtype) else 0.0), (dtype, n)
            assert M.model(x, "VALUE") == (float(np.real(z[-1])), float(np.imag(z[-1]))), (dtype, n)
    # -0.0: the accumulator starts at +0.0
    assert str(M.model(np.full(3, -0.0), "MEAN")[0]) == "0.0" and str(M.model(np.full(3, -0.0), "VALUE")[0]) == "-0.0"


def test_the_exact_sums_are_exact():
    from fractions import Fraction
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, 500) * np.exp2(rng.integers(-200, 200, 500))
    assert M.exact_sum(v) == sum((Fraction(float(t)) for t in v), Fraction(0))
    assert M.exact_sum_squares(v) == sum((Fraction(float(t)) ** 2 for t in v), Fraction(0))
    assert M.exact_sum(np.zeros(3)) == 0 and M.exact_sum_squares(np.array([-0.0, 3.0])) == 9
    assert M.truth(np.array([3, 4], np.int8), "RMS") == (float(np.sqrt(12.5)), 0.0)
    assert M.truth(np.array([[3, 4]], np.int16), "RMS") == (5.0, 0.0) and M.truth(np.array([[3, 4], [1, -1]], np.int16), "MEAN") == (2.0, 1.5)
    assert [M.depth(n) for n in (1, 2, 3, 4, 5, 1 << 22, (1 << 22) + 3)] == [0, 1, 2, 2, 3, 22, 23]


@pytest.mark.parametrize("dtype", M.TYPES)
def test_the_model_lies_within_its_bound_of_the_truth_on_the_gpu_suites_inputs(dev, dtype):
    cases = [c for c in M.all_cases(geometry_of(dev)) if c[0] == dtype]
    assert len(cases) >= 12 + (dtype in M.BIG_TYPES)
    for _, n in cases:
        x = M.make_input(dtype, n)
        assert x.shape[0] == n and x.dtype == M.scalar_of(dtype)
        for mode in M.MODES:
            t, _ = M.case(dtype, n, mode)
            m, lim = M.model(x, mode), M.model_bound(x, mode, t)
            for k in (0, 1):
                assert abs(m[k] - t[k]) <= lim[k], (dtype, n, mode, k, m[k], t[k], lim[k])
            if mode == "VALUE" or M.sum_is_exact(dtype, mode) and mode == "MEAN":
                assert m == t, (dtype, n, mode)
    # the inputs hold what they are meant to
    x = M.make_input(dtype, 257)
    flat = np.asarray(x).reshape(-1)
    if M.scalar_of(dtype).kind == "f":
        big = np.abs(flat.astype(np.float64)) >= 2.0 ** (38 if M.scalar_of(dtype) == np.float32 else 68)      # the cancelling pairs
        assert big.sum() >= 12 and M.exact_sum(flat[big].astype(np.float64)) == 0 and np.abs(flat[~big]).min() < 2.0 ** -20
    else:
        hi = 2 ** 31 - 1 if M.scalar_of(dtype) == np.int64 else np.iinfo(M.scalar_of(dtype)).max
        lo = -hi if M.scalar_of(dtype) == np.int64 else np.iinfo(M.scalar_of(dtype)).min
        assert flat.max() == hi and flat.min() == lo and np.abs(flat.astype(np.float64)).max() < 2.0 ** 31 + 1
