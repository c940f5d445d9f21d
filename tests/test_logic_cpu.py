"""CPU tests of the comparator, bitwise, byte-order and const-arithmetic family: the model against what g++ recorded, the argument
checks of the C ABI that return before a device is touched, the registry and the descriptions of libpcx_logic_blocks.so, the blocks'
defaults and exceptions."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import logic_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "logic_blocks.cpp")
REF = "/root/reference"
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "logic.npz"))
SC = {"float64": 0, "float32": 1, "int64": 2, "int32": 3, "int16": 4, "int8": 5, "uint64": 6, "uint32": 7, "uint16": 8, "uint8": 9}
PATHS = {"/comms/comparator": 2, "/comms/const_comparator": 2, "/comms/const_arithmetic": 3, "/comms/bitwise_unary": 2, "/comms/bitwise_binary": 3,
         "/comms/const_bitwise_binary": 3, "/comms/bitshift": 3, "/comms/byte_order": 1}
REF_DOCS = {"/comms/comparator": "math/Comparator.cpp", "/comms/const_comparator": "math/ConstComparator.cpp",
            "/comms/const_arithmetic": "math/ConstArithmetic.cpp", "/comms/bitwise_unary": "digital/Bitwise.cpp",
            "/comms/bitwise_binary": "digital/Bitwise.cpp", "/comms/const_bitwise_binary": "digital/Bitwise.cpp", "/comms/bitshift": "digital/Bitwise.cpp",
            "/comms/byte_order": "digital/ByteOrder.cpp"}


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ---------------------------------------------------------------- the model is what g++ recorded
@pytest.mark.parametrize("name", M.TYPES)
def test_model_comparisons_equal_the_recorded_ones(name):
    a, b = GOLD["cmp/%s/a" % name], GOLD["cmp/%s/b" % name]
    assert a.dtype == np.dtype(name) and a.size >= 200
    if a.dtype.kind == "f":
        assert np.isnan(a).any() and np.isinf(a).any() and (np.signbit(a) & (a == 0)).any() and np.isnan(b).any()
    else:
        info = np.iinfo(a.dtype)
        assert {info.min, info.max, 0, 1}.issubset(set(a.tolist()))
    for op, key in M.CMP.items():
        assert np.array_equal(M.compare(op, a, b), GOLD["cmp/%s/%s" % (name, key)]), op
        ci = 0
        while "cmpk/%s/%d/k" % (name, ci) in GOLD.files:
            assert np.array_equal(M.compare(op, a, GOLD["cmpk/%s/%d/k" % (name, ci)]), GOLD["cmpk/%s/%d/%s" % (name, ci, key)]), (op, ci)
            ci += 1
        assert ci >= 3
    if a.dtype.kind == "f":      # a NaN constant: only != holds
        assert not GOLD["cmpk/%s/1/EQ" % name].any() and GOLD["cmpk/%s/1/NE" % name].all() and not GOLD["cmpk/%s/1/GE" % name].any()
        zero = a == 0
        assert GOLD["cmpk/%s/0/EQ" % name][zero].all() and (np.signbit(a[zero])).any()       # -0.0 == 0.0


@pytest.mark.parametrize("name", M.INT_TYPES)
def test_model_bitwise_and_shifts_equal_the_recorded_ones(name):
    a, b, k = GOLD["bit/%s/a" % name], GOLD["bit/%s/b" % name], GOLD["bitk/%s/k" % name]
    assert np.array_equal(M.bitwise("NOT", [a]), GOLD["bit/%s/NOT" % name])
    for op in ("AND", "OR", "XOR"):
        assert np.array_equal(M.bitwise(op, [a, b]), GOLD["bit/%s/%s" % (name, op)])
        assert np.array_equal(M.bitwise_const(op, a, k), GOLD["bitk/%s/%s" % (name, op)])
    x = GOLD["shift/%s/a" % name]
    info = np.iinfo(x.dtype)
    assert {info.min, info.max, 0}.issubset(set(x.tolist())) and (info.min == 0 or -1 in x.tolist())
    nbits = 8 * x.dtype.itemsize
    assert GOLD["shift/%s/L" % name].shape == GOLD["shift/%s/R" % name].shape == (nbits, x.size)
    for s in range(nbits):
        assert np.array_equal(M.bitshift(True, x, s), GOLD["shift/%s/L" % name][s]), s
        assert np.array_equal(M.bitshift(False, x, s), GOLD["shift/%s/R" % name][s]), s


@pytest.mark.parametrize("width", [2, 4, 8])
def test_model_byte_reversal_equals_the_recorded_one(width):
    a, want = GOLD["swap/%d/a" % width], GOLD["swap/%d/out" % width]
    assert a.dtype.itemsize == width and np.array_equal(M.byteswap(a), want)
    # the same bytes read as the other types with scalars of this width (a complex element is two scalars)
    for dt in {2: [np.int16], 4: [np.int32, np.float32, np.complex64], 8: [np.int64, np.float64, np.complex128]}[width]:
        assert np.array_equal(bits(M.byteswap(a.view(dt))), bits(want)), dt


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", M.TYPES)
def test_model_const_arithmetic_equals_the_recorded_one(oracle, name, cplx):
    for group in ("ak", "ref"):
        key = "%s/%s/%s" % (group, name, "c" if cplx else "r")
        for op, rec in M.ARITHK.items():
            if group == "ak":
                x, k = GOLD[key + ("/xd" if op == "K/X" else "/x")], GOLD[key + "/k"]
            else:
                x, k = (GOLD[key + "/kbyx_x"], GOLD[key + "/kbyx_k"]) if op[0] == "K" else (GOLD[key + "/xbyk_x"], GOLD[key + "/xbyk_k"])
            assert x.shape == ((x.shape[0], 2) if cplx else (x.shape[0],)) and k.size == (2 if cplx else 1)
            assert np.array_equal(bits(M.arith_const(oracle, op, x, k, cplx)), bits(GOLD["%s/%s" % (key, rec)])), (group, op)
    # the reference test's own numbers (math/TestArithmeticBlocks.cpp:424-508)
    key = "ref/%s/%s" % (name, "c" if cplx else "r")
    assert GOLD[key + "/xbyk_x"].shape[0] == GOLD[key + "/kbyx_x"].shape[0] == 100
    assert GOLD[key + "/xbyk_k"].tolist() == ([3, 2] if cplx else [2]) and GOLD[key + "/kbyx_k"].tolist() == ([102, 101] if cplx else [102])


def test_the_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "logic.npz")) < 420 * 1024


# ---------------------------------------------------------------- the C ABI's argument checks (none of these reaches a device)
def test_c_abi_refuses_what_it_cannot_run(pcx):
    L, lib = pcx._lib.load(), pcx._lib
    x = np.arange(64, dtype=np.uint8)
    y = np.zeros(64, np.uint8)
    px, py = x.ctypes.data, y.ctypes.data
    ptrs = (C.c_void_p * 2)(px, px)

    def refused(rc, word):
        assert rc == lib.ERR_ARG and word in L.pcx_last_error().decode(), (rc, L.pcx_last_error())

    refused(L.pcx_compare(10, lib.CMP_GT, px, px, py, 8), "unsupported type")
    refused(L.pcx_compare(-1, lib.CMP_GT, px, px, py, 8), "unsupported type")
    refused(L.pcx_compare(SC["uint8"], 6, px, px, py, 8), "unknown comparison")
    refused(L.pcx_compare_const(SC["float32"], -1, px, px, py, 8), "unknown comparison")
    refused(L.pcx_compare_const(SC["float32"], lib.CMP_GT, px, None, py, 8), "null constant")
    refused(L.pcx_compare_dev(SC["uint8"], 7, px, px, py, 8, None), "unknown comparison")
    for sc in ("float32", "float64"):
        refused(L.pcx_bitwise(SC[sc], lib.BIT_AND, ptrs, 2, py, 4), "integer types only")
        refused(L.pcx_bitwise_const(SC[sc], lib.BIT_AND, px, px, py, 4), "integer types only")
        refused(L.pcx_bitshift(SC[sc], 1, px, 1, py, 4), "integer types only")
    refused(L.pcx_bitwise(SC["uint8"], 4, ptrs, 2, py, 8), "unknown operation")
    refused(L.pcx_bitwise(SC["uint8"], lib.BIT_XOR, ptrs, 0, py, 8), "no input")
    refused(L.pcx_bitwise(SC["uint8"], lib.BIT_XOR, ptrs, 1, py, 8), "over 1 input")
    refused(L.pcx_bitwise(SC["uint8"], lib.BIT_NOT, ptrs, 2, py, 8), "over 2 input")
    refused(L.pcx_bitwise_dev(SC["uint8"], lib.BIT_NOT, ptrs, 0, py, 8, None), "no input")
    refused(L.pcx_bitwise_const(SC["uint8"], lib.BIT_NOT, px, px, py, 8), "unknown operation")
    for name, nbits in (("int8", 8), ("uint8", 8), ("int16", 16), ("uint32", 32), ("int64", 64)):
        refused(L.pcx_bitshift(SC[name], 1, px, nbits, py, 1), "a shift of %d" % nbits)
        refused(L.pcx_bitshift_dev(SC[name], 0, px, nbits + 5, py, 1, None), "a shift of")
    for w in (0, 1, 3, 16):
        refused(L.pcx_byteswap(w, px, py, 4), "unsupported scalar width")
    refused(L.pcx_arith_const(10, 0, 0, px, px, py, 8), "unsupported type")
    refused(L.pcx_arith_const(SC["int16"], 0, 6, px, px, py, 8), "unknown operation")
    refused(L.pcx_arith_const(SC["int16"], 1, 0, px, None, py, 8), "null constant")
    # the overlap rule is checked before anything is queued
    refused(L.pcx_bitwise_const(SC["uint8"], lib.BIT_AND, px, px, px + 1, 32), "overlaps")
    refused(L.pcx_bitshift(SC["uint16"], 1, px + 2, 1, px, 16), "overlaps")
    refused(L.pcx_byteswap(4, px, px + 4, 8), "overlaps")
    refused(L.pcx_arith_const(SC["float32"], 1, 0, px, px, px + 8, 4), "overlaps")
    refused(L.pcx_compare(SC["float32"], lib.CMP_GT, px, py, px, 8), "overlaps")          # wider scalars: not even at the input's start
    refused(L.pcx_compare_const(SC["int16"], lib.CMP_GT, px, py, px + 3, 8), "overlaps")
    refused(L.pcx_compare(SC["uint8"], lib.CMP_GT, px, py, py + 1, 8), "overlaps")
    ptrs3 = (C.c_void_p * 3)(py, px, py)
    refused(L.pcx_bitwise(SC["uint8"], lib.BIT_XOR, ptrs3, 3, py, 16), "it may be one")          # the output twice among the inputs
    refused(L.pcx_bitwise_dev(SC["uint8"], lib.BIT_XOR, ptrs3, 3, py, 16, None), "it may be one")
    ptrs2 = (C.c_void_p * 3)(py, px, px + 16)
    refused(L.pcx_bitwise(SC["uint8"], lib.BIT_OR, ptrs2, 3, px + 8, 16), "overlaps")
    assert np.array_equal(x, np.arange(64, dtype=np.uint8)) and not y.any()
    # nothing to do: PCX_OK, whatever the pointers
    assert L.pcx_compare(SC["float64"], lib.CMP_NE, None, None, None, 0) == lib.OK
    assert L.pcx_bitwise(SC["uint8"], lib.BIT_XOR, ptrs, 2, None, 0) == lib.OK
    assert L.pcx_bitshift(SC["int8"], 1, None, 7, None, 0) == lib.OK
    assert L.pcx_byteswap(8, None, None, 0) == lib.OK
    assert L.pcx_arith_const_dev(SC["uint64"], 1, lib.ARITHK_K_DIV_X, None, px, None, 0, None) == lib.OK


def test_python_wrappers_name_their_operations(dev, pcx):
    E = pcx._lib.InvalidArgument
    x = np.zeros(4, np.int16)
    for call in (lambda: dev.compare("=>", x, x), lambda: dev.compare_const("<>", x, 1), lambda: dev.bitwise("NAND", [x, x]), lambda: dev.bitwise_const("NOT", x, 1),
                 lambda: dev.arith_const("K+X", x, 1, False), lambda: dev.bitshift(True, x, -1), lambda: dev.bitshift(True, x, 16), lambda: dev.byteswap(x.view(np.int8))):
        with pytest.raises(E):
            call()
    assert set(dev.CMP_OPS) == set(M.CMP) and set(dev.ARITHK_OPS) == set(M.ARITHK) and set(dev.BIT_OPS) == {"NOT", "AND", "OR", "XOR"}


# ---------------------------------------------------------------- the module
def test_registry_has_the_eight_paths_with_their_arities():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("logic") == sorted(PATHS)
    for path, arity in PATHS.items():
        assert B.registry_arity(path, module="logic") == arity, path
    assert B.registry_arity("/comms/arithmetic", module="logic") == -1


EXT_PAIRS = {("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
SETTERS = {"/comms/const_comparator": {("constant", "setConstant", "setter")}, "/comms/const_arithmetic": {("constant", "setConstant", "setter")},
           "/comms/const_bitwise_binary": {("constant", "setConstant", "setter")}, "/comms/bitshift": {("shiftSize", "setShiftSize", "setter")},
           "/comms/byte_order": {("byteOrder", "setByteOrder", "setter")}}
MAKE_ARGS = {"/comms/comparator": ("float64", ">"), "/comms/const_comparator": ("float64", ">"), "/comms/const_arithmetic": ("float32", "X+K", 0.0),
             "/comms/bitwise_unary": ("uint64", "NOT"), "/comms/bitwise_binary": ("uint64", "AND", 2), "/comms/const_bitwise_binary": ("uint64", 0, "AND"),
             "/comms/bitshift": ("uint64", "LEFTSHIFT", 0), "/comms/byte_order": ("uint64",)}


def our_docs():
    return {d["factory"][0]: d for d in parse_docs(open(SRC).read())}


def test_descriptions_match_the_registry_and_the_registered_calls():
    from pothoscomms_amd import blocks as B
    docs = our_docs()
    assert set(docs) == set(PATHS)
    source_calls = registered_calls(open(SRC).read())
    for path, d in docs.items():
        assert len(d["factory"][1]) == PATHS[path], path
        # a block built from the description's own defaults
        defaults = [d["params"][k]["default"].strip('"') for k in d["factory"][1]]
        assert [str(a) if isinstance(a, str) else a for a in MAKE_ARGS[path]] == [t(v) for t, v in zip([type(a) for a in MAKE_ARGS[path]], defaults)], path
        blk = B.make(path, *MAKE_ARGS[path], module="logic")
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
        assert " ".join(d["prose"]).strip() and len(d["category"]) == 1
        assert int(d["params"]["portSlabBytes"]["default"]) == blk.call("getPortSlabBytes") == 64 << 20
        blk.close()


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
@pytest.mark.parametrize("path", sorted(PATHS))
def test_descriptions_have_the_reference_schema_and_their_own_words(path):
    ours = our_docs()[path]
    ref = {d["factory"][0]: d for d in parse_docs(open(os.path.join(REF, REF_DOCS[path])).read())}[path]
    assert ours["title"] == ref["title"] and ours["factory"] == ref["factory"] and ours["category"] == ref["category"]
    assert ours["alias"] == ref["alias"] and ours["keywords"] == ref["keywords"]
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


def test_block_defaults_ports_and_exceptions(pcx):
    from pothoscomms_amd import blocks as B
    E = pcx._lib.InvalidArgument
    # ports: the comparators write int8 of dimension 1 whatever the input's dimension is
    b = B.make("/comms/comparator", "float32", "<=", dimension=3, module="logic")
    assert [p[1:4] for p in b.ports(0)] == [("float32", 3, 12)] * 2 and [p[1:4] for p in b.ports(1)] == [("int8", 1, 1)]
    b = B.make("/comms/const_comparator", "uint16", "!=", dimension=2, module="logic")
    assert [p[1:4] for p in b.ports(0)] == [("uint16", 2, 4)] and [p[1:4] for p in b.ports(1)] == [("int8", 1, 1)]
    assert b.call("constant") == 0 and set(b.calls()) >= {"constant", "setConstant", "probeConstant"}
    b.call("setConstant", 65535)
    assert b.call("constant") == 65535
    b = B.make("/comms/bitwise_binary", "int32", "OR", 5, dimension=3, module="logic")
    assert len(b.ports(0)) == 5 and [p[1:4] for p in b.ports(1)] == [("int32", 3, 12)]
    # constants keep their bits
    for dtype, k in (("int8", -128), ("uint64", (1 << 64) - 1), ("int64", -(1 << 63)), ("uint16", 40000)):
        b = B.make("/comms/const_bitwise_binary", dtype, np.int64(k) if k < (1 << 63) else np.uint64(k), "XOR", module="logic")
        assert b.call("constant") == k
        b = B.make("/comms/const_arithmetic", dtype, "K-X", np.int64(k) if k < (1 << 63) else np.uint64(k), module="logic")
        assert b.call("constant") == k
    b = B.make("/comms/const_arithmetic", "complex_float64", "X/K", 1.5 - 2j, module="logic")
    assert b.call("constant") == 1.5 - 2j
    b = B.make("/comms/const_arithmetic", "float32", "X*K", 0.1, module="logic")
    assert b.call("constant") == float(np.float32(0.1))
    b = B.make("/comms/byte_order", "complex_int16", dimension=2, module="logic")
    assert b.call("getByteOrder") == "Swap Order"
    for order in ("Big Endian", "Little Endian", "Network to Host", "Host to Network", "Swap Order"):
        b.call("setByteOrder", order)
        assert b.call("getByteOrder") == order
    with pytest.raises(E, match="Invalid byte order"):
        b.call("setByteOrder", "big endian")
    assert b.call("getByteOrder") == "Swap Order"
    # the shift size: below the bit width, at construction and afterwards (a RangeException in the reference)
    b = B.make("/comms/bitshift", "int8", "RIGHTSHIFT", 7, module="logic")
    assert b.call("shiftSize") == 7
    with pytest.raises(pcx._lib.PcxError, match=r"Shift size cannot be >= the number of bits \(8\) in the type \(int8\)"):
        b.call("setShiftSize", 8)
    assert b.call("shiftSize") == 7
    with pytest.raises(pcx._lib.PcxError, match="Shift size cannot be >= the number of bits"):
        B.make("/comms/bitshift", "uint32", "LEFTSHIFT", 32, module="logic")
    # what the factories refuse, with the reference's words
    for make, words in ((lambda: B.make("/comms/comparator", "uint8", ">", module="logic"), "unsupported args"),
                        (lambda: B.make("/comms/comparator", "complex_float32", ">", module="logic"), "unsupported args"),
                        (lambda: B.make("/comms/comparator", "float32", "=>", module="logic"), "unsupported args"),
                        (lambda: B.make("/comms/const_comparator", "complex_int8", ">", module="logic"), "unsupported args"),
                        (lambda: B.make("/comms/const_comparator", "int8", "><", module="logic"), "unsupported args"),
                        (lambda: B.make("/comms/const_arithmetic", "float32", "K+X", 1.0, module="logic"), "unsupported args"),
                        (lambda: B.make("/comms/bitwise_unary", "float32", "NOT", module="logic"), "DType: float32, Operation: NOT"),
                        (lambda: B.make("/comms/bitwise_unary", "int8", "AND", module="logic"), "DType: int8, Operation: AND"),
                        (lambda: B.make("/comms/bitwise_binary", "uint8", "NOT", 2, module="logic"), "Operation: NOT"),
                        (lambda: B.make("/comms/bitwise_binary", "uint8", "AND", 1, module="logic"), "numChannels=1"),
                        (lambda: B.make("/comms/bitwise_binary", "uint8", "AND", 0, module="logic"), "numChannels must be 2 or more"),
                        (lambda: B.make("/comms/bitwise_binary", "complex_int8", "AND", 2, module="logic"), "DType: complex_int8"),
                        (lambda: B.make("/comms/const_bitwise_binary", "float64", 1, "AND", module="logic"), "DType: float64"),
                        (lambda: B.make("/comms/bitshift", "int16", "ROTATE", 1, module="logic"), "Operation: ROTATE"),
                        (lambda: B.make("/comms/byte_order", "int8", module="logic"), "Unsupported or invalid type"),
                        (lambda: B.make("/comms/byte_order", "complex_uint8", module="logic"), "Unsupported or invalid type")):
        with pytest.raises(E, match=words):
            make()
    # every type the factories take
    for dtype in M.TYPES:
        B.make("/comms/const_comparator", dtype, "==", module="logic").close()
        for c in ("", "complex_"):
            B.make("/comms/const_arithmetic", c + dtype, "X/K", 1, module="logic").close()
            if dtype not in ("int8", "uint8"):
                B.make("/comms/byte_order", c + dtype, module="logic").close()
        if dtype in M.INT_TYPES:
            for path, args in (("/comms/bitwise_unary", ("NOT",)), ("/comms/bitwise_binary", ("XOR", 3)), ("/comms/const_bitwise_binary", (1, "OR")),
                               ("/comms/bitshift", ("RIGHTSHIFT", 1))):
                B.make(path, dtype, *args, module="logic").close()
        if not dtype.startswith("uint"):
            B.make("/comms/comparator", dtype, "!=", module="logic").close()


def test_signals_and_probes_reach_a_connected_slot():
    """setConstant / setShiftSize emit their signal, the value with it except for the const comparator's"""
    from pothoscomms_amd import blocks as B
    sink = B.make("/comms/bitshift", "uint64", "LEFTSHIFT", 0, module="logic")
    src = B.make("/comms/bitshift", "uint16", "RIGHTSHIFT", 1, module="logic")
    src.connect_signal("shiftSizeChanged", sink, "setShiftSize")
    src.call("setShiftSize", 9)
    assert sink.call("shiftSize") == 9
    k = B.make("/comms/const_bitwise_binary", "uint8", 0, "AND", module="logic")
    k.connect_signal("constantChanged", sink, "setShiftSize")
    k.call("setConstant", 33)
    assert sink.call("shiftSize") == 33
    a = B.make("/comms/const_arithmetic", "int32", "X+K", 0, module="logic")
    a.connect_signal("constantChanged", sink, "setShiftSize")
    a.call("setConstant", 12)
    assert sink.call("shiftSize") == 12
    # the probe: a slot without arguments and the signal it fires, which a slot can be wired to
    assert a.calls()["probeConstant"] == 0 and src.calls()["probeShiftSize"] == 0
    a.connect_signal("constantTriggered", sink, "setShiftSize")
    with pytest.raises(Exception, match="no such signal"):
        a.connect_signal("shiftSizeTriggered", sink, "setShiftSize")
    # the const comparator's signal carries no value: a slot of one argument refuses it
    c = B.make("/comms/const_comparator", "int16", ">", module="logic")
    c.connect_signal("constantChanged", sink, "setShiftSize")
    with pytest.raises(Exception, match="wrong number of arguments"):
        c.call("setConstant", 3)
    assert c.call("constant") == 3


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
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_logic_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"pcxb_make_args", "pcxb_work", "pcxb_work_ports", "pcxb_call_int64", "pcxb_get_complex", "pcxb_registry_path"} <= exported
    assert all(s.startswith("pcxb_") for s in exported), sorted(s for s in exported if not s.startswith("pcxb_"))
