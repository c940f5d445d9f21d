"""/comms/waveform_source and /comms/noise_source without a device: the host-only table builders against the recorded reference
(tests/golden/source.npz, exactly), the numpy walk of tests/source_model.py against every recorded call, the registry, the block
interface, the descriptions and the argument checks of the C ABI."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import source_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "waveform_blocks.cpp")
REF = "/root/reference"
NAMES = ("waveform_source", "noise_source")
PATHS = sorted(p + n for p in ("/blocks/", "/comms/") for n in NAMES)
COMMON_CALLS = {"setDevice": 1, "getDevice": 0, "setPortSlabBytes": 1, "getPortSlabBytes": 0}
WAVE_CALLS = {"setWaveform": 1, "getWaveform": 0, "setOffset": 1, "getOffset": 0, "setAmplitude": 1, "getAmplitude": 0, "setFrequency": 1,
              "getFrequency": 0, "setSampleRate": 1, "getSampleRate": 0, "setResolution": 1, "getResolution": 0}
NOISE_CALLS = {"setWaveform": 1, "getWaveform": 0, "setOffset": 1, "getOffset": 0, "setAmplitude": 1, "getAmplitude": 0, "setMean": 1,
               "getMean": 0, "setB": 1, "getB": 0, "setSeed": 1}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "source.npz"))


def settings_after(dtype, wave, ops, upto):
    """the settings in force after ops[:upto + 1]"""
    ampl, offset = M.ampl_offset(dtype)
    s = dict(wave=wave, rate=1.0, freq=0.0, res=0.0, ampl=complex(*ampl), offset=complex(*offset))
    for op, v in ops[:upto + 1]:
        if op in ("freq", "res"):
            s[op] = v
    return s


# ---- the recording itself
def test_recording_covers_what_it_is_meant_to(golden):
    cases = M.waveform_cases()
    assert len(cases) == 12 * 4 + 3 * 6
    for name, dt, wave, ops in cases:
        out, st = golden["out/" + name], golden["state/" + name]
        assert out.shape == M.shape(dt, sum(v for op, v in ops if op == "work")) and out.dtype == M.np_scalar(dt), name
        assert st.shape == (5 + len(ops), 4), name       # wave, rate, ampl, offset, activate, then the ops
    last = {n: golden["state/" + n][-1] for n, _, _, _ in cases}
    # entries, step mod entries and period as the issue computes them from the reference's size loop
    for dt in M.FURTHER_TYPES:
        for key, entries, step, per in (("matrix/%s/SINE", 4096, 410, 2048), ("neg/%s", 4096, 3072, 4), ("zero/%s", 4096, 0, 1),
                                        ("slow/%s", 262144, 26, 131072), ("slowest/%s", 1 << 20, 1, 1 << 20), ("res/%s", 16384, 1638, 8192),
                                        ("retune/%s", 262144, 26, 131072)):
            e, s, m, _ = (int(v) for v in last[key % dt])
            assert (e, s & (e - 1), m, M.period(e, s)) == (entries, step, entries - 1, per), key % dt
    assert int(last["neg/float64"][1]) == (1 << 64) - 1024          # llround(-0.25 * 4096) as a size_t
    assert str(golden["unachievable"]) == "WaveformSource::updateTable()|step size not achievable"
    assert str(golden["unknown_wave"]) == "WaveformSource::setWaveform(TRIANGLE)|unknown waveform setting"
    for name, dt, wave in M.noise_cases():
        assert golden["out/" + name].shape == M.shape(dt, 500) and golden["state/" + name].shape == (11, 4), name
    assert golden["noise_imag_first"].shape == ()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "source.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "symbols.npz"))


# ---- pcx_waveform_table and the walk
def test_waveform_table_and_walk_reproduce_every_recorded_case(golden, dev):
    for name, dt, wave, ops in M.waveform_cases():
        st, out = golden["state/" + name], golden["out/" + name]
        index, at, table, step = 0, 0, None, None
        for k, (op, v) in enumerate(ops):
            row = st[5 + k]
            if op == "work":
                got, index = M.walk(table, index, step, v)
                assert np.array_equal(got, out[at:at + v]), (name, k)
                at += v
            else:
                table, step = dev.waveform_table(dt, **settings_after(dt, wave, ops, k))
            assert (table.shape[0], step, table.shape[0] - 1, index) == tuple(int(x) for x in row), (name, k)
        assert M.digest(table) == str(golden["sha/" + name]), name
        if "table/" + name in golden.files:
            assert np.array_equal(table, golden["table/" + name]), name


def test_waveform_table_before_any_frequency_and_size_only(pcx, dev):
    L = pcx._lib.load()
    for dt in M.TYPES:
        table, step = dev.waveform_table(dt, "CONST")
        assert table.shape == M.shape(dt, 4096) and step == 0
        one = np.ones(2 if M.is_complex(dt) else 1, table.dtype)
        if M.is_complex(dt):
            one[1] = 0
        assert np.array_equal(table, np.broadcast_to(one if M.is_complex(dt) else one[0], table.shape))
    entries, step = C.c_size_t(), C.c_uint64()
    assert L.pcx_waveform_table(1, 1, 1, 1.0, 1e-4, 0.0, 1.0, 0.0, 0.0, 0.0, None, 0, C.byref(entries), C.byref(step)) == 0
    assert (entries.value, step.value) == (262144, 26)
    buf = (C.c_ubyte * 64)()
    assert L.pcx_waveform_table(1, 1, 1, 1.0, 1e-4, 0.0, 1.0, 0.0, 0.0, 0.0, buf, 4, C.byref(entries), C.byref(step)) == pcx._lib.ERR_ARG


def test_waveform_table_refuses_what_the_reference_refuses(golden, pcx, dev):
    where, what = str(golden["unachievable"]).split("|")
    with pytest.raises(pcx._lib.InvalidArgument, match=what):
        dev.waveform_table("complex_float32", "SINE", freq=1e-7)
    L, err = pcx._lib.load(), pcx._lib.last_error
    entries, step = C.c_size_t(), C.c_uint64()
    for bad in (-1, 4, 99):
        assert L.pcx_waveform_table(1, 1, bad, 1.0, 0.1, 0.0, 1.0, 0.0, 0.0, 0.0, None, 0, C.byref(entries), C.byref(step)) == pcx._lib.ERR_ARG
        assert err() == str(golden["unknown_wave"]).split("|")[1]
    # the step comes first, as in updateTable()
    assert L.pcx_waveform_table(1, 1, 99, 1.0, 1e-7, 0.0, 1.0, 0.0, 0.0, 0.0, None, 0, C.byref(entries), C.byref(step)) == pcx._lib.ERR_ARG
    assert err() == what
    assert L.pcx_waveform_table(1, 1, 1, 1.0, 0.1, 0.0, 1.0, 0.0, 0.0, 0.0, None, 0, None, C.byref(step)) == pcx._lib.ERR_ARG
    assert L.pcx_waveform_table(7, 1, 1, 1.0, 0.1, 0.0, 1.0, 0.0, 0.0, 0.0, None, 0, C.byref(entries), C.byref(step)) == pcx._lib.ERR_ARG
    with pytest.raises(ValueError, match="unknown waveform setting"):
        dev.waveform_table("float32", "TRIANGLE")


# ---- pcx_noise
def test_noise_tables_and_windows_reproduce_every_recorded_case(golden, dev):
    for name, dt, wave in M.noise_cases():
        gen = dev.NoiseGenerator(M.NOISE_SEED)
        table = gen.table(dt, wave, mean=M.NOISE_MEAN, b=M.NOISE_B, ampl=100.0 if M.is_integer(dt) else 1.0)
        assert M.digest(table) == str(golden["sha/" + name]), name
        if "table/" + name in golden.files:
            assert np.array_equal(table, golden["table/" + name]), name
        out, st = golden["out/" + name], golden["state/" + name]
        index = 0
        for k, n in enumerate(M.NOISE_CALLS):
            draw = gen.next_offset()
            assert 0 <= draw < 4096
            got, index = M.walk(table, index + draw, 1, n)
            assert np.array_equal(got, out[100 * k:100 * k + n]), (name, k)
            assert index == int(st[6 + k][3]), (name, k)
        gen.close()


def test_the_draw_order_is_the_recorded_one(golden):
    text = open(os.path.join(ROOT, "pothoscomms_amd", "csrc", "pcx_src_api.hip")).read()
    assert ("constexpr bool kImagFirst = %s;" % ("true" if bool(golden["noise_imag_first"]) else "false")) in text


def test_noise_generators_without_a_seed_differ_and_unknown_waves_are_refused(pcx, dev):
    a, b = dev.NoiseGenerator(), dev.NoiseGenerator()
    assert not np.array_equal(a.table("float64", "NORMAL"), b.table("float64", "NORMAL"))
    s, t = dev.NoiseGenerator(7), dev.NoiseGenerator(7)
    assert np.array_equal(s.table("complex_int8", "UNIFORM", b=100.0), t.table("complex_int8", "UNIFORM", b=100.0))
    with pytest.raises(ValueError, match="unknown waveform setting"):
        a.table("float32", "CAUCHY")
    L = pcx._lib.load()
    buf = (C.c_ubyte * (4096 * 16))()
    for bad in (-1, 4):
        assert L.pcx_noise_table(a._h, 1, 0, bad, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, buf) == pcx._lib.ERR_ARG and pcx._lib.last_error() == "unknown waveform setting"
    assert L.pcx_noise_table(None, 1, 0, 0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, buf) == pcx._lib.ERR_ARG
    assert L.pcx_noise_table(a._h, 1, 0, 0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, None) == pcx._lib.ERR_ARG
    assert L.pcx_noise_next_offset(None, None) == pcx._lib.ERR_ARG and L.pcx_noise_create(0, 0, None) == pcx._lib.ERR_ARG
    for g in (a, b, s, t):
        g.close()


# ---- the model
def test_walk_wraps_modulo_two_to_the_64():
    table = np.arange(8, dtype=np.int16)
    out, index = M.walk(table, (1 << 64) - 3, 1, 6)
    assert list(out) == [5, 6, 7, 0, 1, 2] and index == 3
    out, index = M.walk(table, 1, (1 << 64) - 2, 4)         # a step of -2
    assert list(out) == [1, 7, 5, 3] and index == (1 - 8) & M.M64
    assert [M.period(4096, s) for s in (0, 1, 410, 16, 2048, 4096, (1 << 64) - 1024, 4097)] == [1, 4096, 2048, 256, 2, 1, 4, 4096]


# ---- the C ABI (no device is touched)
def test_abi_argument_errors_come_before_any_device_call(pcx):
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    err = pcx._lib.last_error
    buf = (C.c_ubyte * (16 << 10))()
    h, idx = C.c_void_p(), C.c_uint64()
    a, b, s = C.c_size_t(), C.c_size_t(), C.c_int()
    assert L.pcx_source_create(1, 1, None) == E
    for bad in (-1, 6, 9, 10):          # the unsigned types are arithmetic's only
        assert L.pcx_source_create(bad, 0, C.byref(h)) == E and "unsupported type" in err()
    assert L.pcx_source_set_table(None, buf, 16, 1) == E and "null handle" in err()
    assert L.pcx_source_get_index(None, C.byref(idx)) == E and L.pcx_source_set_index(None, 0) == E
    assert L.pcx_source_get_geometry(None, C.byref(a), C.byref(b), C.byref(s)) == E
    assert L.pcx_source_generate(None, buf, 4) == E and "null handle" in err()
    assert L.pcx_source_generate_dev(None, buf, 4, None) == E and "null handle" in err()
    for scalar, cplx, es in ((1, 1, 8), (5, 0, 1), (0, 1, 16)):
        assert L.pcx_source_create(scalar, cplx, C.byref(h)) == 0
        try:
            assert L.pcx_source_get_geometry(h, C.byref(a), C.byref(b), C.byref(s)) == 0 and (a.value, b.value, s.value) == ((16 << 10) // es, 0, 0)
            # the size comes before the table pointer
            for bad in (0, 3, 12, 4095, 4097, (1 << 20) + 1, 1 << 21, 1 << 40):
                assert L.pcx_source_set_table(h, None, bad, 1) == E and "power of two of at most 1048576" in err(), bad
            assert L.pcx_source_set_table(h, None, 16, 1) == E and "null table" in err()
            # n == 0 comes before everything but the handle; the index stays
            assert L.pcx_source_set_index(h, 77) == 0
            assert L.pcx_source_generate(h, None, 0) == 0 and L.pcx_source_generate_dev(h, None, 0, None) == 0
            assert L.pcx_source_get_index(h, C.byref(idx)) == 0 and idx.value == 77
            assert L.pcx_source_generate(h, None, 4) == E and "null buffer" in err()
            assert L.pcx_source_generate_dev(h, None, 4, None) == E and "null buffer" in err()
            # no table yet
            assert L.pcx_source_generate(h, buf, 4) == pcx._lib.ERR_STATE and "no table" in err()
            assert L.pcx_source_get_index(h, None) == E and L.pcx_source_get_geometry(h, C.byref(a), None, C.byref(s)) == E
        finally:
            assert L.pcx_source_destroy(h) == 0
    assert L.pcx_source_destroy(None) == 0 and L.pcx_noise_destroy(None) == 0


def test_header_declares_the_family_and_the_binding_covers_it(pcx):
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    family = sorted(set(re.findall(r"PCX_API\s+int\s+(pcx_(?:source|noise|waveform)_\w+)\s*\(", src)))
    assert family == sorted(["pcx_source_" + n for n in ("create", "destroy", "set_table", "get_index", "set_index", "get_geometry", "generate",
                                                         "generate_dev")] + ["pcx_waveform_table"] +
                            ["pcx_noise_" + n for n in ("create", "destroy", "table", "next_offset")])
    assert sorted(n for n in pcx._lib.SIGNATURES if re.match(r"pcx_(source|noise|waveform)_", n)) == family
    L = pcx._lib
    assert (L.WAVE_CONST, L.WAVE_SINE, L.WAVE_RAMP, L.WAVE_SQUARE) == (0, 1, 2, 3)
    assert (L.NOISE_UNIFORM, L.NOISE_NORMAL, L.NOISE_LAPLACE, L.NOISE_POISSON, L.NOISE_ENTRIES) == (0, 1, 2, 3, 4096)
    for text in ("THE CARRIED INDEX IS HOST\n * STATE", "step size not achievable", "unknown waveform setting", "#define PCX_NOISE_ENTRIES 4096"):
        assert text in src, text
    blk = open(os.path.join(ROOT, "include", "pcx_blocks.h")).read()
    assert "pcxb_call_complex" in blk and "pcxb_get_complex" in blk and "nin = 0" in blk


# ---- the blocks (libpcx_waveform_blocks.so)
def test_module_registry_holds_exactly_the_four_paths():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("waveform") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="waveform") == 1
        assert path not in B.registry_paths()
        for other in ("filter", "envelope", "iir", "digital", "correlator", "symbol", "repack"):
            assert path not in B.module_registry_paths(other)


def test_the_twelve_types_are_accepted_and_others_refused():
    from pothoscomms_amd import _lib, blocks as B
    for path in PATHS:
        for dt in M.TYPES:
            b = B.make(path, dt, module="waveform")
            assert b.out_dtype == dt and b.in_dtype is None and b.ports(0) == [] and [p[1] for p in b.ports(1)] == [dt]
            b.close()
        for bad in ("uint8", "uint16", "complex_uint32", "uint64"):
            with pytest.raises(_lib.InvalidArgument, match="unsupported type"):
                B.make(path, bad, module="waveform")
        with pytest.raises(_lib.InvalidArgument, match="unsupported type"):
            B.make(path, "float32", dimension=2, module="waveform")


def test_fresh_blocks_answer_the_constructors_values():
    from pothoscomms_amd import blocks as B
    for prefix in ("/comms/", "/blocks/"):
        w = B.make(prefix + "waveform_source", "complex_float32", module="waveform")
        assert w.calls() == dict(COMMON_CALLS, **WAVE_CALLS)
        assert (w.call("getWaveform"), w.call("getOffset"), w.call("getAmplitude")) == ("CONST", 0j, 1 + 0j)
        assert (w.call("getSampleRate"), w.call("getFrequency"), w.call("getResolution")) == (1.0, 0.0, 0.0)
        n = B.make(prefix + "noise_source", "int16", module="waveform")
        assert n.calls() == dict(COMMON_CALLS, **NOISE_CALLS)
        assert (n.call("getWaveform"), n.call("getOffset"), n.call("getAmplitude"), n.call("getMean"), n.call("getB")) == ("NORMAL", 0j, 1 + 0j, 0.0, 1.0)
        for b in (w, n):
            # the complex setters round-trip; nothing is built or refused while the block is not active
            for name in ("Offset", "Amplitude"):
                for v in (0.25 - 0.5j, -3e9 + 1e-300j, 7.0):
                    b.call("set" + name, v)
                    assert b.call("get" + name) == complex(v)
            b.call("setWaveform", "NO SUCH WAVE")
            assert b.call("getWaveform") == "NO SUCH WAVE"
            assert b.call("getPortSlabBytes") == 64 << 20
            b.call("setPortSlabBytes", 1 << 20)
            assert b.call("getPortSlabBytes") == 1 << 20
        w.call("setFrequency", 1e-7)            # not achievable, but not looked at yet
        w.call("setSampleRate", 48e3)
        w.call("setResolution", 0.5)
        assert (w.call("getFrequency"), w.call("getSampleRate"), w.call("getResolution")) == (1e-7, 48e3, 0.5)
        n.call("setMean", -2.5)
        n.call("setB", 0.125)
        n.call("setSeed", 20261018)
        assert (n.call("getMean"), n.call("getB")) == (-2.5, 0.125)
        w.close()
        n.close()


def _docs():
    return {d["factory"][0].split("/")[2]: d for d in parse_docs(open(SRC).read())}


def test_descriptions_match_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = _docs()
    assert sorted(d["factory"] for d in docs.values()) == sorted(("/comms/" + n, ["dtype"]) for n in NAMES)
    assert registered_calls(text) == set(COMMON_CALLS) | set(WAVE_CALLS) | set(NOISE_CALLS)
    want = {"waveform_source": {("rate", "setSampleRate"), ("wave", "setWaveform"), ("offset", "setOffset"), ("ampl", "setAmplitude"),
                                ("freq", "setFrequency"), ("res", "setResolution")},
            "noise_source": {("wave", "setWaveform"), ("offset", "setOffset"), ("ampl", "setAmplitude"), ("mean", "setMean"), ("b", "setB")}}
    for name, d in docs.items():
        pairs = set()
        for kind, fn, keys in d["calls"]:
            assert len(keys) == 1 and fn in (WAVE_CALLS if name == "waveform_source" else NOISE_CALLS) or fn in COMMON_CALLS, fn
            pairs.add((keys[0], fn, kind))
        assert pairs == {(k, f, "setter") for k, f in want[name]} | {("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}
        # `fast` of the noise source is a parameter without a call, in the reference as here
        assert set(d["params"]) == {k for k, _, _ in pairs} | {"dtype"} | ({"fast"} if name == "noise_source" else set())
        assert d["alias"] == ["/blocks/" + name]
        for key, p in d["params"].items():
            assert " ".join(p["desc"]).strip() and p["default"] is not None, (name, key)
            if p["options"]:
                assert p["default"] in p["options"]
        assert " ".join(d["prose"]).strip()
    assert docs["waveform_source"]["params"]["wave"]["options"] == ['"CONST"', '"SINE"', '"RAMP"', '"SQUARE"']
    assert docs["noise_source"]["params"]["wave"]["options"] == ['"UNIFORM"', '"NORMAL"', '"LAPLACE"', '"POISSON"']
    assert "setSeed" in " ".join(docs["noise_source"]["prose"])


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
def test_descriptions_have_the_reference_schema_and_their_own_words():
    files = {"waveform_source": "WaveformSource.cpp", "noise_source": "NoiseSource.cpp"}
    for name, ours in _docs().items():
        ref = parse_docs(open(os.path.join(REF, "waveform", files[name])).read())[0]
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


def test_the_extension_is_marked_and_written_down():
    text = open(SRC).read()
    assert len(re.findall(r"// EXTENSION", text)) >= 3 and "setSeed" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "/comms/waveform_source" in open(os.path.join(ROOT, "README.md")).read()
