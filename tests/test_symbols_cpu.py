"""CPU suite of /comms/symbol_mapper, /comms/symbol_slicer, /comms/differential_encoder and /comms/differential_decoder: the model
(tests/symbol_model.py) against itself and against the recorded reference outputs (tests/golden/symbols.npz), the C ABI's argument
checks, the registry of libpcx_symbol_blocks.so, the four descriptions and the blocks' defaults.  No device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import symbol_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "symbol_blocks.cpp")
REF = "/root/reference"
NAMES = ["differential_decoder", "differential_encoder", "symbol_mapper", "symbol_slicer"]
PATHS = sorted(p + n for p in ("/blocks/", "/comms/") for n in NAMES)
ARITY = {"differential_decoder": 0, "differential_encoder": 0, "symbol_mapper": 1, "symbol_slicer": 1}
REF_FILES = {"symbol_mapper": "SymbolMapper.cpp", "symbol_slicer": "SymbolSlicer.cpp", "differential_encoder": "DifferentialEncoder.cpp",
             "differential_decoder": "DifferentialDecoder.cpp"}
# the issue's table: symbols -> does the step equal (in + last) mod min(symbols, 256) for all 65536 pairs
PLAN_TABLE = [(1, True), (2, True), (255, True), (256, True), (257, False), (300, False), (510, False), (511, True), (65536, True),
              (2 ** 32 - 511, True), (2 ** 32 - 510, False), (2 ** 32 - 256, True), (2 ** 32 - 1, False)]
COMMON_CALLS = {"setDevice": 1, "getDevice": 0, "setPortSlabBytes": 1, "getPortSlabBytes": 0}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "symbols.npz"))


# ---- the model
def test_plan_table_is_reproduced():
    for symbols, scan in PLAN_TABLE:
        assert (M.encoder_plan(symbols) == M.SCAN) == scan, symbols
    for symbols in range(1, 257):
        assert M.encoder_plan(symbols) == M.SCAN, symbols
    for symbols in range(257, 511):
        assert M.encoder_plan(symbols) == M.SERIAL, symbols


def test_the_two_encoder_formulations_agree_where_the_plan_is_scan():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, 3000, dtype=np.uint8)
    for symbols in [1, 2, 3, 4, 7, 100, 255, 256, 511, 65536, 2 ** 32 - 511, 2 ** 32 - 256]:
        assert M.encoder_plan(symbols) == M.SCAN
        for last in (0, 1, 200, 255):
            a, la = M.encoder_steps(x, symbols, last)
            b, lb = M.encoder_scan(x, symbols, last)
            assert np.array_equal(a, b) and la == lb, (symbols, last)
    # and they differ where it is not: the plan is no formality
    for symbols in (257, 300, 2 ** 32 - 1):
        a, _ = M.encoder_steps(x, symbols, 0)
        b, _ = M.encoder_scan(x, symbols, 0)
        assert not np.array_equal(a, b), symbols


def test_decoder_undoes_encoder_for_clean_symbols():
    rng = np.random.default_rng(2)
    for symbols in (1, 2, 4, 7, 256):
        x = rng.integers(0, symbols, 2000).astype(np.uint8)
        enc, _ = M.encoder(x, symbols)
        dec, _ = M.decoder(enc, symbols)
        assert np.array_equal(dec, x), symbols


def test_mapper_mask_and_errors():
    assert [M.mapper_mask(n) for n in (1, 2, 4, 256, 512, 65536)] == [0, 1, 3, 255, 255, 255]
    with pytest.raises(ValueError, match="nonzero"):
        M.mapper_mask(0)
    with pytest.raises(ValueError, match="power of two"):
        M.mapper_mask(6)


def test_slicer_special_distances_give_symbol_0_and_first_wins():
    f = np.float32
    assert list(M.slicer(np.array([f(np.nan), f(np.inf)]), np.array([f(0), f(1)]))) == [0, 0]
    assert list(M.slicer(np.array([f(5), f(1), f(1)]), np.array([f(1)]))) == [1]
    assert list(M.slicer(np.array([f(-1), f(1)]), np.array([f(0), f(np.nan), f(np.inf)]))) == [0, 0, 0]
    # a distance equal to FLT_MAX never wins
    assert list(M.slicer(np.array([f(0), f(M.FLT_MAX)]), np.array([f(M.FLT_MAX)]))) == [1]
    assert list(M.slicer(np.array([f(3), f(0)]), np.array([f(M.FLT_MAX)]))) == [0]
    # doubles that the narrowing to float makes equal: the first wins
    m = np.array([1.0 + 2.0 ** -40, 1.0])
    assert list(M.slicer(m, np.array([0.0]))) == [0]
    # an index beyond 255 is stored modulo 256
    big = np.arange(300, dtype=np.int32) * 10
    assert list(M.slicer(big, np.array([2990, 2560, 10], dtype=np.int32))) == [299 & 255, 0, 1]


def test_model_equals_every_fixture_case(golden):
    cases = [str(k) for k in golden["cases"]]
    assert len(cases) == 160
    for key in cases:
        kind = key.split("/")[0]
        if kind == "map":
            got = M.mapper(golden["m/" + key], golden["map_in"])
            assert got.dtype == golden["out/" + key].dtype and np.array_equal(got.view(np.uint8), golden["out/" + key].view(np.uint8)), key
        elif kind == "slice":
            assert np.array_equal(M.slicer(golden["m/" + key], golden["in/" + key]), golden["out/" + key]), key
        else:
            symbols, decode = int(key.split("/")[1]), kind == "dec"
            out, last = M.run_coder(decode, M.coder_ops(symbols), golden["code_in"])
            state = golden["state/" + key]
            assert np.array_equal(out, golden["out/" + key]) and last == int(state[0]), key
            if not decode:
                assert M.encoder_plan(symbols) == int(state[1]), key
                out2, last2 = M.run_coder(False, M.coder_ops(symbols), golden["code_in"], step_form=True)
                assert np.array_equal(out2, out) and last2 == last, key


def test_fixture_covers_what_it_is_meant_to(golden):
    cases = {str(k) for k in golden["cases"]}
    for scalar, cplx in M.TYPES:
        t = M.type_name(scalar, cplx)
        assert {"map/%s/%d" % (t, n) for n in (1, 2, 4, 256, 512)} <= cases
        want = {"bpsk", "rand16", "pts256", "pts300", "dup"} | ({"qpsk"} if cplx else set()) | ({"naninf"} if "float" in scalar else set())
        assert {"slice/%s/%s" % (t, m) for m in want} <= cases
        x = golden["in/slice/%s/pts300" % t]
        if "float" in scalar:
            assert np.isnan(x).any() and np.isinf(x).any() and (np.abs(x[np.isfinite(x) & (x != 0)]) < 1.2e-38).any()
        else:
            assert int(np.abs(x.astype(np.float64)).max()) >= {"int64": 2 ** 61, "int32": 2 ** 29, "int16": 2 ** 14, "int8": 64}[scalar]
        assert golden["out/slice/%s/pts300" % t].max() > 0
    assert (golden["map_in"] > 127).any() and (golden["code_in"] > 250).any()
    for s in M.CODER_SYMBOLS:
        assert {"enc/%d" % s, "dec/%d" % s} <= cases


# ---- the C ABI (no device is touched)
def test_abi_argument_errors_come_before_any_device_call(pcx):
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    err = pcx._lib.last_error
    one = (C.c_float * 8)(1, 0, 0, 0, 0, 0, 0, 0)
    buf = (C.c_ubyte * 64)()
    n = C.c_size_t()
    for fam in ("pcx_mapper", "pcx_slicer"):
        f = lambda name: getattr(L, fam + "_" + name)      # noqa: E731
        h = C.c_void_p()
        assert f("create")(pcx.F32, 0, None) == E
        assert f("create")(99, 0, C.byref(h)) == E and "unsupported type" in err()
        assert f("create")(pcx._lib.U8, 0, C.byref(h)) == E and "unsupported type" in err()       # bad scalar: the unsigned types
        assert f("set_map")(None, one, 1) == E and "null handle" in err()
        assert f("get_map")(None, None, 0, C.byref(n)) == E
        assert f("process")(None, buf, buf, 4) == E and "null handle" in err()
        assert f("process_dev")(None, buf, buf, 4, None) == E and "null handle" in err()
        assert f("create")(pcx.F32, 1, C.byref(h)) == 0
        try:
            # the constructor's map: {1}
            got = (C.c_float * 4)()
            assert f("get_map")(h, got, 2, C.byref(n)) == 0 and (n.value, got[0], got[1]) == (1, 1.0, 0.0)
            assert f("set_map")(h, one, 0) == E and "Map must be nonzero size" in err()
            assert f("set_map")(h, None, 0) == E and "Map must be nonzero size" in err()
            assert f("set_map")(h, None, 2) == E and "null map" in err()
            if fam == "pcx_mapper":
                for bad in (3, 6, 255, 300):
                    assert f("set_map")(h, one, bad) == E and "Map must be a power of two in length" in err(), bad
            assert f("get_map")(h, got, 2, C.byref(n)) == 0 and (n.value, got[0], got[1]) == (1, 1.0, 0.0)        # refused: unchanged
            assert f("process")(h, None, None, 0) == 0 and f("process_dev")(h, None, None, 0, None) == 0
            assert f("process")(h, None, buf, 4) == E and "null buffer" in err()
            assert f("process_dev")(h, buf, None, 4, None) == E and "null buffer" in err()
            # overlap: 4 input elements against the output (the mapper reads 4 bytes and writes 32, the slicer the other way round)
            base = C.addressof(buf)
            for in_off, out_off in ((0, 0), (0, 2), (2, 0)):
                assert f("process_dev")(h, C.c_void_p(base + in_off), C.c_void_p(base + out_off), 4, None) == E and "overlaps" in err()
                assert f("process")(h, C.c_void_p(base + in_off), C.c_void_p(base + out_off), 4) == E and "overlaps" in err()
        finally:
            assert f("destroy")(h) == 0
    g = [C.c_size_t() for _ in range(4)]
    assert L.pcx_slicer_get_geometry(None, *[C.byref(v) for v in g]) == E

    h = C.c_void_p()
    assert L.pcx_diffcode_create(0, None) == E
    sym, plan, last = C.c_uint32(), C.c_int(), C.c_ubyte(9)
    assert L.pcx_diffcode_set_symbols(None, 2) == E and "null handle" in err()
    assert L.pcx_diffcode_set_symbols(None, 0) == E and "null handle" in err()
    assert L.pcx_diffcode_get_symbols(None, C.byref(sym)) == E
    assert L.pcx_diffcode_get_plan(None, C.byref(plan)) == E
    assert L.pcx_diffcode_get_state(None, C.byref(last)) == E
    assert L.pcx_diffcode_reset(None) == E
    assert L.pcx_diffcode_get_geometry(None, None) == E
    assert L.pcx_diffcode_process(None, buf, buf, 4) == E and "null handle" in err()
    assert L.pcx_diffcode_process_dev(None, buf, buf, 4, None) == E and "null handle" in err()
    for decode in (0, 1):
        assert L.pcx_diffcode_create(decode, C.byref(h)) == 0
        try:
            assert L.pcx_diffcode_get_symbols(h, C.byref(sym)) == 0 and sym.value == 2
            assert L.pcx_diffcode_get_plan(h, C.byref(plan)) == 0 and plan.value == pcx._lib.DIFF_SCAN
            assert L.pcx_diffcode_set_symbols(h, 300) == 0
            assert L.pcx_diffcode_get_plan(h, C.byref(plan)) == 0
            assert plan.value == (pcx._lib.DIFF_SCAN if decode else pcx._lib.DIFF_SERIAL)
            assert L.pcx_diffcode_set_symbols(h, 0) == E and "symbols cannot be 0" in err()
            assert L.pcx_diffcode_get_symbols(h, C.byref(sym)) == 0 and sym.value == 300                # refused: kept
            assert L.pcx_diffcode_process(h, None, None, 0) == 0 and L.pcx_diffcode_process_dev(h, None, None, 0, None) == 0
            assert L.pcx_diffcode_process(h, None, buf, 4) == E and "null buffer" in err()
            base = C.addressof(buf)
            for in_off, out_off in ((0, 2), (2, 0), (0, 3)):
                assert L.pcx_diffcode_process_dev(h, C.c_void_p(base + in_off), C.c_void_p(base + out_off), 4, None) == E and "overlaps" in err()
                assert L.pcx_diffcode_process(h, C.c_void_p(base + in_off), C.c_void_p(base + out_off), 4) == E and "overlaps" in err()
        finally:
            assert L.pcx_diffcode_destroy(h) == 0


def test_overlap_refusals_name_the_block_and_come_before_any_device_call(pcx):
    """The rule of in and out on fabricated addresses, which are never dereferenced: the mapper and the slicer refuse every shared byte,
    out == in included (their element sizes differ); the coders refuse everything but out == in.  One byte shared at either end is
    refused, with the handle's own text, by the host and the device entry point alike."""
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    err = pcx._lib.last_error
    base, n = 1 << 40, 1 << 20
    for fam, text, nin, nout in (("pcx_mapper", "symbol mapper: out overlaps in", n, 16 * n), ("pcx_slicer", "symbol slicer: out overlaps in", 16 * n, n)):
        f = lambda name: getattr(L, fam + "_" + name)      # noqa: E731
        h = C.c_void_p()
        assert f("create")(pcx.F64, 1, C.byref(h)) == 0
        try:
            # the same buffer, one input element in, the last byte of in, the last byte of out
            for out in (base, base + nin // n, base + nin - 1, base - nout + 1):
                assert f("process_dev")(h, C.c_void_p(base), C.c_void_p(out), n, None) == E and err() == text, (fam, out - base)
                assert f("process")(h, C.c_void_p(base), C.c_void_p(out), n) == E and err() == text, (fam, out - base)
        finally:
            assert f("destroy")(h) == 0
    text = "differential coder: out overlaps in (in place means out == in)"
    for decode in (0, 1):
        h = C.c_void_p()
        assert L.pcx_diffcode_create(decode, C.byref(h)) == 0
        try:
            for out in (base + 1, base + n - 1, base - n + 1):
                assert L.pcx_diffcode_process_dev(h, C.c_void_p(base), C.c_void_p(out), n, None) == E and err() == text, out - base
                assert L.pcx_diffcode_process(h, C.c_void_p(base), C.c_void_p(out), n) == E and err() == text, out - base
        finally:
            assert L.pcx_diffcode_destroy(h) == 0


def test_encoder_plan_of_the_handle_follows_the_table(dev):
    c = dev.DifferentialCoder()
    assert (c.symbols(), c.plan(), c.decode) == (2, dev._lib.DIFF_SCAN, False)
    for symbols, scan in PLAN_TABLE:
        c.set_symbols(symbols)
        assert c.symbols() == symbols and (c.plan() == dev._lib.DIFF_SCAN) == scan, symbols
    with pytest.raises(ValueError, match="symbols cannot be 0"):
        c.set_symbols(0)
    assert c.symbols() == PLAN_TABLE[-1][0]
    c.close()
    d = dev.DifferentialCoder(decode=True, symbols=300)
    assert (d.symbols(), d.plan()) == (300, dev._lib.DIFF_SCAN)
    d.close()
    tile, slc = dev.DifferentialCoder.geometry()
    assert tile % 64 == 0 and slc % tile == 0 and slc <= 64 << 20


def test_python_handles_keep_maps_in_the_stream_types_layout(dev):
    big = np.array([2 ** 62 + 1, -(2 ** 62) - 3, 7, 0], dtype=np.int64)
    for cls in (dev.SymbolMapper, dev.SymbolSlicer):
        h = cls("int64", big)
        assert np.array_equal(h.map(), big)               # beyond 2^53: exact
        h.close()
        h = cls("complex_int16", [1 + 2j, -3 - 4j])
        assert h.map().tolist() == [[1, 2], [-3, -4]]
        with pytest.raises(ValueError, match="Map must be nonzero size"):
            h.set_map([])
        h.close()
        h = cls()
        assert h.map().tolist() == [[1.0, 0.0]] and (h.scalar, h.is_complex) == (dev.F32, True)
        h.close()
    m = dev.SymbolMapper("float32")
    with pytest.raises(ValueError, match="power of two"):
        m.set_map([1, 2, 3])
    m.set_map(np.arange(512))
    assert m.map().shape == (512,)
    m.close()
    s = dev.SymbolSlicer("complex_float64", np.arange(300))
    lane, group, onchip, slc = s.geometry()
    assert group % lane == 0 and onchip >= 256 and slc % group == 0 and s.map().shape == (300, 2)
    s.close()


def test_header_declares_the_families_and_the_binding_covers_them(pcx):
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    want = {"pcx_mapper_": ("create", "destroy", "set_map", "get_map", "process", "process_dev"),
            "pcx_slicer_": ("create", "destroy", "set_map", "get_map", "get_geometry", "process", "process_dev"),
            "pcx_diffcode_": ("create", "destroy", "set_symbols", "get_symbols", "get_plan", "get_geometry", "get_state", "reset", "process",
                              "process_dev")}
    for prefix, names in want.items():
        family = sorted(set(re.findall(r"PCX_API\s+int\s+(%s\w+)\s*\(" % prefix, src)))
        assert family == sorted(prefix + n for n in names)
        assert sorted(n for n in pcx._lib.SIGNATURES if n.startswith(prefix)) == family
    assert "PCX_DIFF_SCAN = 0" in src and "PCX_DIFF_SERIAL = 1" in src


# ---- the blocks (libpcx_symbol_blocks.so)
def test_module_registry_holds_exactly_the_eight_paths():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("symbol") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="symbol") == ARITY[path.split("/")[2]]
        assert path not in B.registry_paths()
        for other in ("filter", "envelope", "iir", "digital", "correlator"):
            assert path not in B.module_registry_paths(other)


def test_fresh_blocks_answer_the_constructors_values():
    from pothoscomms_amd import _lib, blocks as B
    for prefix in ("/comms/", "/blocks/"):
        for name in ("differential_encoder", "differential_decoder"):
            b = B.make(prefix + name, module="symbol")
            assert (b.in_dtype, b.out_dtype, b.call("getSymbols")) == ("uint8", "uint8", 2)
            assert b.calls() == dict(COMMON_CALLS, setSymbols=1, getSymbols=0)
            b.call("setSymbols", 300)
            assert b.call("getSymbols") == 300
            for zero in (0, 1 << 32, 5 << 32):                   # a size_t that narrows to 0
                with pytest.raises(_lib.InvalidArgument, match="symbols cannot be 0"):
                    b.call("setSymbols", zero)
            assert b.call("getSymbols") == 300
            b.call("setSymbols", (1 << 32) + 7)                  # narrows to 7, as the reference's uint32_t member does
            assert b.call("getSymbols") == 7
            out, consumed, produced, _, _ = b.work(np.zeros(0, np.uint8), 16)
            assert (out.size, consumed, produced) == (0, 0, 0)
            b.close()
        for name, dtype in (("symbol_mapper", "complex_float32"), ("symbol_slicer", "int16"), ("symbol_mapper", "int64"),
                            ("symbol_slicer", "complex_float64")):
            b = B.make(prefix + name, dtype, module="symbol")
            want = (("uint8", dtype) if name == "symbol_mapper" else (dtype, "uint8"))
            assert (b.in_dtype, b.out_dtype) == want
            assert b.calls() == dict(COMMON_CALLS, setMap=1, getMap=0)
            assert b.call("getMap").tolist() == [1.0]
            with pytest.raises(_lib.InvalidArgument, match="Map must be nonzero size"):
                b.call("setMap", [])
            if name == "symbol_mapper":
                with pytest.raises(_lib.InvalidArgument, match="Map must be a power of two in length"):
                    b.call("setMap", [1, 2, 3])
            else:
                b.call("setMap", [1, 2, 3])
                assert b.call("getMap").tolist() == [1.0, 2.0, 3.0]
            assert b.call("getMap").tolist() in ([1.0], [1.0, 2.0, 3.0])
            if dtype.startswith("complex"):
                b.call("setMap", [-1 - 1j, -1 + 1j, 1 + 1j, 1 - 1j])
                assert b.call("getMap", True).tolist() == [-1 - 1j, -1 + 1j, 1 + 1j, 1 - 1j]
            else:
                b.call("setMap", [0, 1, 3, 2])
                assert b.call("getMap").tolist() == [0.0, 1.0, 3.0, 2.0]
            assert b.call("getPortSlabBytes") == 64 << 20
            b.close()
    for name in ("symbol_mapper", "symbol_slicer"):
        for bad in ("uint8", "complex_uint16"):
            with pytest.raises(_lib.InvalidArgument, match="unsupported type"):
                B.make("/comms/" + name, bad, module="symbol")


def _docs():
    return {d["factory"][0].split("/")[2]: d for d in parse_docs(open(SRC).read())}


def test_descriptions_match_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert sorted(d["factory"] for d in docs) == sorted(("/comms/" + n, ["dtype"] if ARITY[n] else []) for n in NAMES)
    calls = registered_calls(text)
    assert calls == {"setMap", "getMap", "setSymbols", "getSymbols", "setDevice", "getDevice", "setPortSlabBytes", "getPortSlabBytes"}
    for name, d in _docs().items():
        pairs = set()
        for kind, fn, keys in d["calls"]:
            assert fn in calls and len(keys) == 1, fn
            pairs.add((keys[0], fn, kind))
        own = ("map", "setMap", "setter") if ARITY[name] else ("symbols", "setSymbols", "setter")
        assert pairs == {own, ("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}, name
        assert set(d["params"]) == {k for k, _, _ in pairs} | set(d["factory"][1])
        assert d["alias"] == ["/blocks/" + name] and "/Digital" in d["category"]
        for key, p in d["params"].items():
            assert " ".join(p["desc"]).strip() and p["default"] is not None, (name, key)
            if p["options"] and key != "map":
                assert p["default"] in p["options"]
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

