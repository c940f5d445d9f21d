"""CPU tests of the special-function family (gamma, lngamma, erf, erfc, beta, modf): the fixture tests/golden/specfn.npz against itself,
against the derived bound of beta and against the numpy model of modf; the argument checks of the C ABI that return before a device is
touched; the registry and the descriptions of libpcx_special_blocks.so; ports, names and refusals of the blocks."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import specfn_model as S
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "special_blocks.cpp")
REF = "/root/reference"
GOLD = np.load(S.GOLD_PATH)
F64, F32, I32 = 0, 1, 3
PATHS = {"/comms/gamma": 1, "/comms/lngamma": 1, "/comms/erf": 1, "/comms/erfc": 1, "/comms/beta": 1, "/comms/modf": 1}
REF_DOCS = {"gamma": "Gamma.cpp", "lngamma": "Gamma.cpp", "erf": "ErrorFunction.cpp", "erfc": "ErrorFunction.cpp", "beta": "Beta.cpp", "modf": "ModF.cpp"}
FACTORY = {"/comms/gamma": "gammaFactory", "/comms/lngamma": "lnGammaFactory", "/comms/erf": "erfFactory", "/comms/erfc": "erfcFactory",
           "/comms/beta": "betaFactory", "/comms/modf": "modfFactory"}


# ---------------------------------------------------------------- the fixture
def test_fixture_holds_every_case_and_its_conditions():
    expected = set()
    for fn in S.FUNCS:
        for tname in S.TYPES:
            key = S.case_key(fn, tname)
            expected |= {key + "/ord", key + "/spec"} | (set() if fn == "MODF" else {key + "/e_ref"}) | ({key + "/large"} if fn == "BETA" else set())
            ord_, spec = GOLD[key + "/ord"], GOLD[key + "/spec"]
            rows = 4 if fn == "BETA" else 3
            assert ord_.dtype == spec.dtype == np.dtype(tname) and ord_.shape[0] == spec.shape[0] == rows and 190 <= ord_.shape[1] <= 210, key
            assert np.isfinite(ord_).all(), key
            if fn == "MODF":
                continue
            ref, cr = ord_[-2], ord_[-1]
            d = S.ulp_distance(ref, cr)
            assert int(d.max()) == int(GOLD[key + "/e_ref"]), key
            if fn == "BETA":            # the reference stays within the bound derived from its own expression, in the units of its type
                assert (d <= S.beta_bounds(ord_[0], ord_[1], np.dtype(tname).type)).all(), key
            else:
                assert d.max() <= 4, (key, d.max())
            sref, scr = spec[-2], spec[-1]
            settled = np.isfinite(sref) & (sref != 0)
            assert np.isnan(scr[~settled]).all() and np.isfinite(scr[settled]).all(), key
            if fn != "BETA":            # finite results of special inputs lie as close to the truth as the ordinary ones
                assert S.ulp_distance(sref[settled], scr[settled]).max(initial=0) <= 4, key
    assert set(GOLD.files) == expected


def _has(values, wanted):
    have = {v.tobytes() for v in values}
    return all(np.array(w, dtype=values.dtype).tobytes() in have or (np.isnan(w) and np.isnan(values).any()) for w in wanted)


def test_fixture_domains_and_special_groups():
    for tname in S.TYPES:
        g = lambda fn, part="ord": GOLD["%s/%s/%s" % (fn, tname, part)]
        x = g("GAMMA")[0]
        assert ((x > 0.01) & (x < 20)).sum() == 150 and ((x > -6) & (x < 0)).sum() == 50 and (np.abs(x[x < 0] - np.round(x[x < 0])) > 0.09).all()
        x = g("LNGAMMA")[0]
        assert (((x > 0.01) & (x < 0.75)) | ((x > 1.25) & (x < 1.75)) | ((x > 2.5) & (x < 20))).all()
        assert (np.abs(g("ERF")[0]) < 6).all() and g("ERFC")[0].min() > -6 and 8 < g("ERFC")[0].max() < (9 if tname == "float32" else 25)
        assert tname == "float32" or g("ERFC")[0].max() > 20
        a, b = g("BETA")[:2]
        assert ((a > 0.01) & (a < 20) & (b > 0.01) & (b < 20)).all() and abs(np.corrcoef(a, b)[0, 1]) < 0.3
        x = g("MODF")[0]
        assert (np.abs(x) < 2.0 ** 20).all() and (x < 0).any() and (x > 0).any() and (np.abs(x) < 1).any()
        fi = np.finfo(np.dtype(tname))
        common = [0.0, -0.0, np.inf, -np.inf, np.nan, fi.tiny, -fi.tiny, fi.max, -fi.max, fi.smallest_subnormal, -fi.smallest_subnormal,
                  1.0, -1.0, 0.5, -0.5, 2.0, 3.0, -2.0, -3.0]
        for fn in S.FUNCS:
            assert _has(g(fn, "spec")[0], common), (fn, tname)
        assert _has(g("BETA", "spec")[1], common) and _has(g("BETA", "spec")[0], [171.5, 1e10])
        assert not _has(g("LNGAMMA", "spec")[0], [-2.5]) and _has(g("LNGAMMA", "spec")[0], [-1.5, -3.75, 100.5, -100.5, 1e10])
    tab = lambda fn, tname: dict(zip(GOLD["%s/%s/spec" % (fn, tname)][0].tolist(), GOLD["%s/%s/spec" % (fn, tname)][1].tolist()))
    # overflow and underflow of gamma, on both sides, with the signs the poles leave
    g64, g32 = tab("GAMMA", "float64"), tab("GAMMA", "float32")
    assert np.isfinite(g64[171.5]) and g64[171.7] == np.inf and np.isfinite(g32[34.5]) and g32[35.5] == np.inf
    assert g64[-170.5] != 0 and g64[-190.5] == 0 and g32[-50.5] == 0 and np.isnan(g64[-2.0]) and np.isnan(g32[-np.inf]) and g64[np.inf] == np.inf
    x, ref, _ = GOLD["GAMMA/float64/spec"]
    assert ref[0] == np.inf and ref[1] == -np.inf and x[1] == 0 and np.signbit(x[1])                  # tgamma(+-0) = +-inf
    # lgamma's poles and infinities are +inf, its zeros at 1 and 2 are +0
    l64 = tab("LNGAMMA", "float64")
    assert l64[-np.inf] == l64[np.inf] == l64[-2.0] == l64[0.0] == np.inf and l64[1.0] == 0 and l64[2.0] == 0 and np.isfinite(l64[2.5e305])
    assert np.isfinite(tab("LNGAMMA", "float32")[float(np.float32(4e36))])
    # erf keeps the sign of a zero; erfc underflows between 26.5 and 27.5 (float64) and between 9.5 and 10.5 (float32)
    x, ref, _ = GOLD["ERF/float32/spec"]
    assert ref[1] == 0 and np.signbit(ref[1]) and not np.signbit(ref[0]) and tab("ERF", "float64")[-np.inf] == -1
    c64, c32 = tab("ERFC", "float64"), tab("ERFC", "float32")
    assert c64[26.5] > 0 and c64[27.5] == 0 and c32[9.5] > 0 and c32[10.5] == 0 and c64[-np.inf] == 2
    # beta loses the sign of a negative argument: B(-0.5, 1) is -2, the expression gives +2
    b64 = {(a, b): r for a, b, r in zip(*GOLD["BETA/float64/spec"][:3].tolist())}
    assert b64[(-0.5, 1.0)] == 2.0 == b64[(0.5, 1.0)] and np.isnan(b64[(-1.0, 1.0)]) and b64[(0.0, 1.0)] == np.inf and np.isnan(b64[(np.inf, 1.0)])
    # modf at an integer, at an infinity and beyond the last fraction
    for tname, last in (("float32", 8388607.5), ("float64", 4503599627370495.5)):
        x, ip, fp = GOLD["MODF/%s/spec" % tname]
        at = lambda v: [i for i in range(x.size) if x[i:i + 1].tobytes() == np.array([v], x.dtype).tobytes()][0]
        assert fp[at(-2.0)] == 0 and np.signbit(fp[at(-2.0)]) and ip[at(-2.0)] == -2 and not np.signbit(fp[at(3.0)])
        assert fp[at(-np.inf)] == 0 and np.signbit(fp[at(-np.inf)]) and ip[at(-np.inf)] == -np.inf and fp[at(np.inf)] == 0 and ip[at(np.inf)] == np.inf
        assert np.signbit(ip[at(-0.5)]) and ip[at(-0.5)] == 0 and fp[at(-0.5)] == -0.5 and fp[at(last)] == 0.5 and fp[at(1e10)] == 0
        assert np.isnan(ip[at(np.nan)]) and np.isnan(fp[at(np.nan)])


def test_beta_large_group_straddles_the_threshold():
    for tname in S.TYPES:
        a, b, ref, cr = GOLD["BETA/%s/large" % tname]
        x, y = np.maximum(a, b), np.minimum(a, b)
        assert a.dtype == np.dtype(tname) and 60 <= a.size <= 70 and (a > b).any() and (b > a).any()
        assert (x < 1024).sum() >= 3 and (x == 1024).any() and (x > 1024).sum() >= 50 and x.max() > 1e11 and ((y > 0.01) & (y < 20)).all()
        assert np.isfinite(cr).all() and (cr >= np.finfo(np.dtype(tname)).tiny).all()
    # what the term-by-term expression costs there: the reference's float32 results are off by far more than any bar
    a, b, ref, cr = GOLD["BETA/float32/large"]
    assert S.ulp_distance(ref, cr).max() > 1000


def test_the_fixture_is_small():
    assert os.path.getsize(S.GOLD_PATH) < 512 * 1024


def test_modf_model_equals_the_recorded_bits():
    for tname in S.TYPES:
        for part in ("ord", "spec"):
            x, ip, fp = GOLD["MODF/%s/%s" % (tname, part)]
            got_i, got_f = S.modf_model(x)
            for got, ref in ((got_i, ip), (got_f, fp)):
                keep = ~np.isnan(ref)
                assert got.dtype == ref.dtype and np.array_equal(np.isnan(got), np.isnan(ref)) and keep.sum() >= 20
                assert np.array_equal(got[keep].view(np.uint8), ref[keep].view(np.uint8)), (tname, part)


def test_beta_bound_is_the_formula():
    """one input by hand: la = lb = ln gamma(0.5) = 0.5724, lab = ln gamma(1) = 0"""
    la = 0.5723649429247001
    u = 2.0 ** -53                      # the unit of a double in [0.5, 1)
    e = 16.5 * (u + u + 0) + 2 * u / 2 + 2 * u / 2          # la + lb and la + lb - lab are 1.1447, in [1, 2): a unit of 2^-52
    assert S.beta_bound(la, la, 0.0, np.float64) == int(np.ceil(2.0 ** 53 * e)) + 4 == 35 + 4
    assert S.beta_bound(la, la, 0.0, np.float32) == 39
    assert S.beta_bounds(np.array([0.5]), np.array([0.5]), np.float64)[0] == 39


# ---------------------------------------------------------------- the C ABI's argument checks (none of these reaches a device)
def test_c_abi_refuses_what_it_cannot_run(pcx):
    L, lib = pcx._lib.load(), pcx._lib
    x = np.arange(64, dtype=np.float32)
    y = np.zeros(64, np.float32)
    z = np.zeros(64, np.float32)
    px, py, pz = x.ctypes.data, y.ctypes.data, z.ctypes.data
    F = lib.SPEC_FN

    def refused(rc, word):
        assert rc == lib.ERR_ARG and word in L.pcx_last_error().decode(), (rc, L.pcx_last_error())

    for sc in (I32, 2, 9, 10, -1):
        refused(L.pcx_specfn(sc, F["GAMMA"], px, py, 8), "unsupported type")
        refused(L.pcx_specfn_dev(sc, F["ERFC"], px, py, 8, None), "unsupported type")
        refused(L.pcx_beta(sc, px, py, pz, 8), "unsupported type")
        refused(L.pcx_beta_dev(sc, px, py, pz, 8, None), "unsupported type")
        refused(L.pcx_modf(sc, px, py, pz, 8), "unsupported type")
        refused(L.pcx_modf_dev(sc, px, py, pz, 8, None), "unsupported type")
    for fn in (-1, 4, 5, 16, 48, 1000):
        refused(L.pcx_specfn(F32, fn, px, py, 8), "unknown function")
        refused(L.pcx_specfn_dev(F64, fn, px, py, 8, None), "unknown function")
    refused(L.pcx_specfn(F32, F["ERF"], px, None, 8), "null buffer")
    refused(L.pcx_specfn_dev(F32, F["ERF"], None, py, 8, None), "null buffer")
    for trio in ((None, py, pz), (px, None, pz), (px, py, None)):
        refused(L.pcx_beta(F32, *trio, 8), "null buffer")
        refused(L.pcx_beta_dev(F64, *trio, 8, None), "null buffer")
        refused(L.pcx_modf(F32, *trio, 8), "null buffer")
        refused(L.pcx_modf_dev(F64, *trio, 8, None), "null buffer")
    # the overlap rules are checked before anything is queued
    refused(L.pcx_specfn(F32, F["GAMMA"], px, px + 4, 8), "overlaps")
    refused(L.pcx_specfn_dev(F64, F["LNGAMMA"], px + 8, px, 4, None), "overlaps")
    refused(L.pcx_beta(F32, px, py, px + 4, 8), "overlaps")
    refused(L.pcx_beta(F32, py, px, px + 4, 8), "overlaps")
    refused(L.pcx_beta_dev(F32, px, px + 4, px, 8, None), "overlaps")                  # out is in0, and cuts into in1
    refused(L.pcx_modf(F32, px, px + 4, py, 8), "overlaps")
    refused(L.pcx_modf(F32, px, py, px + 16, 8), "overlaps")
    refused(L.pcx_modf_dev(F64, px, py, py + 8, 4, None), "overlaps")                  # one output on the other
    refused(L.pcx_modf_dev(F32, px, py, py, 8, None), "overlaps")
    refused(L.pcx_modf(F32, px, px, px, 8), "overlaps")
    assert np.array_equal(x, np.arange(64, dtype=np.float32)) and not y.any() and not z.any()
    # nothing to do: PCX_OK, whatever the pointers
    assert L.pcx_specfn(F64, F["ERF"], None, None, 0) == lib.OK and L.pcx_specfn_dev(F32, F["GAMMA"], None, None, 0, None) == lib.OK
    assert L.pcx_beta(F32, None, None, None, 0) == lib.OK and L.pcx_beta_dev(F64, px, px + 4, px, 0, None) == lib.OK
    assert L.pcx_modf(F64, None, None, None, 0) == lib.OK and L.pcx_modf_dev(F32, px, px, px, 0, None) == lib.OK
    assert F == {"GAMMA": 0, "LNGAMMA": 1, "ERF": 2, "ERFC": 3}


def test_python_wrappers_refuse_what_the_calls_refuse(dev, pcx):
    E = pcx._lib.InvalidArgument
    x = np.ones(8, np.float32)
    for call in (lambda: dev.special_fn("DIGAMMA", x), lambda: dev.special_fn("BETA", x), lambda: dev.special_fn("ERF", x.astype(np.int32)),
                 lambda: dev.special_fn("GAMMA", x, out=x[1:]), lambda: dev.special_fn("GAMMA", x[:7], out=x[1:]),
                 lambda: dev.beta(x, x[:4]), lambda: dev.beta(x, x.astype(np.float64)), lambda: dev.beta(x.astype(np.int32), x.astype(np.int32)),
                 lambda: dev.beta(x[:6], x[:6], out=x[1:7]),
                 lambda: dev.modf(x.astype(np.complex64)), lambda: dev.modf(x[:6], out_int=x[1:7]), lambda: dev.modf(x, out_int=x, out_frac=x),
                 lambda: dev.modf(x, out_frac=np.zeros(4, np.float32))):
        with pytest.raises(E):
            call()
    assert np.array_equal(x, np.ones(8, np.float32))


# ---------------------------------------------------------------- the module
def make(path, *args, **kw):
    from pothoscomms_amd import blocks as B
    return B.make(path, *args, module="special", **kw)


def test_registry_has_the_six_paths_with_arity_one():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("special") == sorted(PATHS)
    for path, arity in PATHS.items():
        assert B.registry_arity(path, module="special") == arity == 1, path
        assert B.registry_arity(path.replace("/comms/", "/blocks/"), module="special") == -1         # none of the six has an alias
    assert B.registry_arity("/comms/exp", module="special") == -1 and B.registry_arity("/comms/gamma", module="math") == -1


EXT_PAIRS = {("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}


def our_docs():
    return {d["factory"][0]: d for d in parse_docs(open(SRC).read())}


def test_descriptions_match_the_registry_and_the_registered_calls():
    docs = our_docs()
    assert set(docs) == set(PATHS)
    source_calls = registered_calls(open(SRC).read())
    for path, d in docs.items():
        assert d["factory"][1] == ["dtype"], path
        assert d["params"]["dtype"]["default"] == '"float64"'
        blk = make(path, "float64")                 # a block built from the description's own default
        calls = blk.calls()
        pairs = set()
        for kind, fn, keys in d["calls"]:
            assert fn in source_calls and calls.get(fn) == 1 and len(keys) == 1, (path, fn)
            pairs.add((keys[0], fn, kind))
        assert pairs == EXT_PAIRS, path
        assert set(d["params"]) == {"dtype", "device", "portSlabBytes"}, path
        for key, p in d["params"].items():
            assert p["default"] is not None and " ".join(p["desc"]).strip(), (path, key)
        assert " ".join(d["prose"]).strip() and d["category"] == ["/Math"] and d["alias"] == []
        assert int(d["params"]["portSlabBytes"]["default"]) == blk.call("getPortSlabBytes") == 64 << 20
        blk.close()
    assert docs["/comms/modf"]["params"]["dtype"]["widget"] == "DTypeChooser(float=1,dim=1)"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
@pytest.mark.parametrize("path", sorted(PATHS))
def test_descriptions_have_the_reference_schema_and_their_own_words(path):
    ours = our_docs()[path]
    ref = {d["factory"][0]: d for d in parse_docs(open(os.path.join(REF, "math", REF_DOCS[path.rsplit("/", 1)[1]])).read())}[path]
    assert ours["title"] == ref["title"] and ours["factory"] == ref["factory"] and ours["category"] == ref["category"]
    assert ours["alias"] == ref["alias"] == [] and ours["keywords"] == ref["keywords"]
    ext = {"device", "portSlabBytes"}
    assert [k for k in ours["order"] if k not in ext] == ref["order"] and set(ours["order"]) - set(ref["order"]) == ext
    assert {(fn, tuple(k), kind) for kind, fn, k in ours["calls"] if k[0] not in ext} == {(fn, tuple(k), kind) for kind, fn, k in ref["calls"]} == set()
    for key, rp in ref["params"].items():
        for field in ("name", "default", "options", "widget", "preview", "tab", "units"):
            assert ours["params"][key][field] == rp[field], (key, field)

    def sentences(doc):
        text = " ".join(doc["prose"]) + " " + " ".join(" ".join(p["desc"]) for p in doc["params"].values())
        text = re.sub(r"<[^>]+>", " ", text)
        return {re.sub(r"\s+", " ", s).strip().lower() for s in re.split(r"[.;:]\s", text) if len(s.split()) >= 6}
    assert sentences(ours) and not (sentences(ours) & sentences(ref))


def test_ports_names_dimensions_and_refusals(pcx):
    E = pcx._lib.InvalidArgument
    for path in PATHS:
        for dtype, size in (("float32", 4), ("float64", 8)):
            b = make(path, dtype, dimension=3)
            ins, outs = b.ports(0), b.ports(1)
            assert [p[1:4] for p in ins] == [(dtype, 3, 3 * size)] * (2 if path == "/comms/beta" else 1), path
            assert [p[1:4] for p in outs] == [(dtype, 3, 3 * size)] * (2 if path == "/comms/modf" else 1), path
            assert [p[0] for p in ins] == (["0", "1"] if path == "/comms/beta" else ["0"]), path
            assert [p[0] for p in outs] == (["int", "frac"] if path == "/comms/modf" else ["0"]), path
            assert set(b.calls()) >= {"setDevice", "getDevice", "setPortSlabBytes", "getPortSlabBytes"}
            b.close()
        # the words the reference's factories use for a type they do not know
        for dtype in ("int32", "complex_float32", "uint8", "int64"):
            with pytest.raises(E, match=r"%s\(.*unsupported type" % FACTORY[path]):
                make(path, dtype)


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
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_special_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"pcxb_make_args", "pcxb_work", "pcxb_work_ports", "pcxb_call_double", "pcxb_get_double", "pcxb_registry_path"} <= exported
    assert all(s.startswith("pcxb_") for s in exported), sorted(s for s in exported if not s.startswith("pcxb_"))


def test_the_shared_kernel_has_one_home():
    """mathfn_kernel, apply1 and launch_fn live in fn_kernel.hpp alone; both sources include it and the Makefile knows it as a dependency"""
    csrc = os.path.join(ROOT, "pothoscomms_amd", "csrc")
    read = lambda f: open(os.path.join(csrc, f)).read()
    for name in ("void mathfn_kernel(", "T apply1(", "int launch_fn("):
        assert name in read("fn_kernel.hpp") and name not in read("mathfn.hip") and name not in read("specfn.hip"), name
    assert '#include "fn_kernel.hpp"' in read("mathfn.hip") and '#include "fn_kernel.hpp"' in read("specfn.hip")
    mk = read("Makefile")
    assert mk.count("$(HERE)fn_kernel.hpp") == 2 and " specfn.hip" in mk and re.search(r"^MODULES\s*:=.*\bspecial\b", mk, flags=re.M)
