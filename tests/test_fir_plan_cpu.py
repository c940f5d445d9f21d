"""CPU check of the FIR planner (csrc/fir_plan.hpp, plain C++): which plan serves (element type, taps, L, M, K, requested algorithm).
A host compiler builds tests/fir_plan_main.cpp over the handle's own header, once plain and once under the address and
undefined-behaviour sanitizers, and the program runs as a child process.  Two checks: every row of tests.fir_plans.PLANS resolves to the
algorithm and plan the row names (the table tests/test_fir_plans_gpu.py holds the device to), and a sweep over every accepted type, the
resampling factors and each tap-count bound of the header keeps the planner's invariants.  No device is touched."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from tests.fir_plans import PLANS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pothoscomms_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

with open(os.path.join(INCLUDE, "pcx.h")) as _f:
    _H = _f.read()
PLAN = {name: int(v) for name, v in re.findall(r"PCX_FIR_PLAN_(\w+) = (\d+)", _H)}
PLAN_NAME = {v: k for k, v in PLAN.items()}
ALGO = {name: int(v) for name, v in re.findall(r"PCX_FIR_(AUTO|DIRECT|OLS_FFT|EXACT) = (\d+)", _H)}
SCALAR = {name: int(v) for name, v in re.findall(r"PCX_(F64|F32|I64|I32|I16|I8) = (\d+)", _H)}
DTYPE = {"float32": "F32", "float64": "F64", "int64": "I64", "int32": "I32", "int16": "I16", "int8": "I8"}
REQUESTS = ("AUTO", "DIRECT", "OLS_FFT", "EXACT")                    # the order the program resolves them in
TIME_DOMAIN = {"CF32_DIRECT_TILE", "DOT2", "SLIDE", "GENERIC"}
FREQ_DOMAIN = set(PLAN) - TIME_DOMAIN - {"NONE", "CF32_OLS4096_GATED"}  # (the gated name is the call's, never the planner's)

SAN = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_the_header_enums_were_read():
    assert len(PLAN) == 21 and len(ALGO) == 4 and len(SCALAR) == 6


def build(tmp, name, extra):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                       ["-I" + CSRC, "-I" + INCLUDE, os.path.join(ROOT, "tests", "fir_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def planner(request, tmp_path_factory):
    """configurations -> the program's answers, one dict per configuration"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = build(str(tmp_path_factory.mktemp("fir_plan")), "fir_plan_" + request.param, tuple(SAN) if request.param == "sanitizers" else ())

    def run(configs):
        text = "".join("%d %d %d %d %d %d %d %d\n" % c for c in configs)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(configs)
        out = []
        for line in lines:
            head, tail = line.split("|")
            K, ols_plan, auto_min, td_algo, td_plan, parts, log2n, fold = (int(v) for v in head.split())
            t = [int(v) for v in tail.split()]
            out.append(dict(K=K, ols_plan=PLAN_NAME[ols_plan], auto_min=auto_min, td_algo=td_algo, td_plan=PLAN_NAME[td_plan], parts=parts,
                            log2n=log2n, fold=fold,
                            resolved={req: (t[3 * i], PLAN_NAME[t[3 * i + 1]], bool(t[3 * i + 2])) for i, req in enumerate(REQUESTS)}))
        return out
    return run


def row_config(row):
    cplx = row.dtype.startswith("complex_")
    scalar = SCALAR[DTYPE[row.dtype[len("complex_"):] if cplx else row.dtype]]
    ctaps = row.taps == "COMPLEX"
    exact = row.name != "ci16 sliding ||h_q||^2 above 2^44"
    taps16 = row.dtype in ("complex_int16", "complex_int8") and ctaps and row.tapgen in ("q16", "normal")
    return (scalar, cplx, ctaps, row.ntaps, row.L, row.M, taps16, exact)


def test_every_row_of_the_plan_table(planner):
    got = planner([row_config(r) for r in PLANS])
    wrong = []
    for row, g in zip(PLANS, got):
        algo, plan, refused = g["resolved"][row.algo]
        if refused or (algo, plan) != (ALGO[row.want], row.plan):
            wrong.append((row.name, algo, plan, refused))
    assert not wrong, wrong


FACTORS = (1, 2, 3, 4, 16, 64, 65, 65535, 65536)
# every tap count fir_plan.hpp names: the AUTO thresholds (2, 4, 16, 24, 32, 48, 64, 96), the plans' ranges (2049, 4097, 8193), the packed
# kernel's 12000, the last K whose time-domain tile fits (5216) and where K - 1 passes 2048 / L for L = 16, 4, 2 (129, 513, 1025)
BOUNDS = (1, 2, 4, 16, 24, 32, 48, 64, 96, 129, 513, 1025, 2049, 4097, 5216, 8193, 12000)
KS = sorted({k for b in BOUNDS for k in (b - 1, b, b + 1) if k >= 1})


def sweep_configs():
    out = []
    for name, (cplx, ctaps), L, M, K in itertools.product(SCALAR, ((0, 0), (1, 0), (1, 1)), FACTORS, FACTORS, KS):
        integer16 = name in ("I16", "I8")
        for ntaps in sorted({K * L, (K - 1) * L + 1}):                  # the longest and the shortest tap vector with K taps a row
            out.append((SCALAR[name], cplx, ctaps, ntaps, L, M, 0, 1))
            if integer16:
                out.append((SCALAR[name], cplx, ctaps, ntaps, L, M, 0, 0))
            if integer16 and ctaps and L == 1 and M == 1:
                out.append((SCALAR[name], cplx, ctaps, ntaps, L, M, 1, 1))
    return out


def family_fits(plan, scalar, cplx):
    f32, dbl = scalar == SCALAR["F32"], scalar in (SCALAR["F64"], SCALAR["I16"], SCALAR["I8"])
    if plan.startswith("CF32_"):
        return f32 and cplx
    if plan.startswith("F32_"):
        return f32 and not cplx
    if plan.startswith("UPOLS_"):
        return f32
    if plan.startswith("CF64_"):
        return dbl and cplx
    if plan.startswith("REAL64_"):
        return dbl and not cplx
    return plan in ("NONE", "DOT2", "SLIDE", "GENERIC")


def test_sweep_invariants(planner):
    configs = sweep_configs()
    got = planner(configs)
    runs = {}      # the configuration without its tap count -> AUTO's plan for ascending K
    taken = set()
    for c, g in zip(configs, got):
        scalar, cplx, ctaps, ntaps, L, M, taps16, exact = c
        assert g["K"] == -(-ntaps // L), c
        assert g["ols_plan"] in FREQ_DOMAIN | {"NONE"} and g["td_plan"] in TIME_DOMAIN, (c, g)
        assert g["td_algo"] in (ALGO["DIRECT"], ALGO["EXACT"]), (c, g)
        have = g["ols_plan"] != "NONE"
        # AUTO is never refused, and takes ols_plan exactly from auto_min_taps on within the plan's own range
        want = (ALGO["OLS_FFT"], g["ols_plan"], False) if have and g["K"] >= g["auto_min"] else (g["td_algo"], g["td_plan"], False)
        assert g["resolved"]["AUTO"] == want, (c, g)
        # a forced OLS_FFT is refused or returns ols_plan, never a time-domain plan
        algo, plan, refused = g["resolved"]["OLS_FFT"]
        assert refused == (not have) and algo == ALGO["OLS_FFT"] and plan == g["ols_plan"], (c, g)
        # DIRECT and EXACT never return a frequency-domain plan
        for req in ("DIRECT", "EXACT"):
            algo, plan, refused = g["resolved"][req]
            assert algo == ALGO[req] and plan in TIME_DOMAIN and not refused, (c, g)
        # the plan's family fits the element type
        for req in REQUESTS:
            assert family_fits(g["resolved"][req][1], scalar, cplx), (c, g)
        ragged = ntaps != g["K"] * L
        runs.setdefault((scalar, cplx, ctaps, L, M, taps16, exact, ragged), []).append(g["resolved"]["AUTO"][1])
        taken.add(g["resolved"]["AUTO"][1])
    # monotone: over ascending K, AUTO enters a frequency-domain plan once and does not come back to it after leaving
    for key, plans in runs.items():
        seen = [p for p, _ in itertools.groupby(plans)]
        fd = [p for p in seen if p in FREQ_DOMAIN]
        assert len(fd) == len(set(fd)), (key, seen)
    assert taken == FREQ_DOMAIN | TIME_DOMAIN        # the sweep reaches every plan
