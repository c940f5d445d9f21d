"""GPU tests of the exp, log, pow, root and trigonometric maps (csrc/mathfn.hip) through the C ABI, host and device forms, and through
the blocks of libpcx_math_blocks.so.

THE BARS.  The reference's results are glibc's, the device's are the ROCm device library's; both are held to the
correctly rounded value `cr` of the exact expression (tests/golden/mathfn.npz, mpmath), in units in the last place.
  * sqrt in both types and rsqrt in both types have one right answer and must equal the recorded `ref` wherever that is not a NaN.
  * every other float32 result is the double expression rounded once: within 1 unit of cr.
  * a float64 result is the device library's.  BAR64 below is the double-precision bound of the OpenCL C specification's table of
    built-in accuracy -- quoted from memory, no copy of the table was at hand: exp exp2 exp10 expm1 log log2 log10 3; log1p cbrt 2;
    sin cos asin acos sinh cosh asinh acosh 4; tan atan tanh atanh 5; pow 16; division and sqrt correctly rounded -- plus 1 per
    further rounded step of a composite expression: 1 / f(x) is +1; f(1 / x) is +1 (the fixture's script holds the condition number of
    f at 1 / x to 2 on the domain, so the half unit of the division arrives as at most one unit); sinc = sin, one division: 4 + 1;
    sigmoid = exp, one sum, one division: 3 + 1 + 1; logN = two logarithms and a division: 3 + 3 + 1; expN and nth_root are pow: 16
    (the mirrored root multiplies by +-1, which is exact).
  * special inputs: a NaN where ref is a NaN (payloads are not compared), the same value with the same sign where ref is an infinity
    or a zero, the ordinary bar elsewhere.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import mathfn_model as M

pytestmark = pytest.mark.gpu

GOLD = np.load(M.GOLD_PATH)
BAR64 = {"EXP": 3, "EXP2": 3, "EXP10": 3, "EXPM1": 3, "LOG": 3, "LOG2": 3, "LOG10": 3, "LOG1P": 2, "SQRT": 0, "CBRT": 2, "RSQRT": 0,
         "SINC": 4 + 1, "SIGMOID": 3 + 1 + 1,
         "COS": 4, "SIN": 4, "TAN": 5, "SEC": 4 + 1, "CSC": 4 + 1, "COT": 5 + 1,
         "ACOS": 4, "ASIN": 4, "ATAN": 5, "ASEC": 4 + 1, "ACSC": 4 + 1, "ACOT": 5 + 1,
         "COSH": 4, "SINH": 4, "TANH": 5, "SECH": 4 + 1, "CSCH": 4 + 1, "COTH": 5 + 1,
         "ACOSH": 4, "ASINH": 4, "ATANH": 5, "ASECH": 4 + 1, "ACSCH": 4 + 1, "ACOTH": 5 + 1,
         "POW": 16, "EXPN": 16, "LOGN": 3 + 3 + 1, "NTH_ROOT": 16}
EXACT = ("SQRT", "RSQRT")
KBLOCK, GUARD, FILL = 256, 64, 0xA5


def bar(fn, dt):
    return 0 if fn in EXACT else 1 if dt == np.float32 else BAR64[fn]


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def check_case(fn, got_ord, got_spec, key):
    """hold one function's results on the ordinary and the special inputs to the bars above; prints the largest distance first"""
    x, ref, cr = GOLD[key + "/ord"]
    sx, sref, scr = GOLD[key + "/spec"]
    b = bar(fn, x.dtype.type)
    d = M.ulp_distance(got_ord, cr)
    worst = int(np.argmax(d))
    print("%-26s largest distance from the truth %g (bar %d) at x = %r; from the reference %g" % (key, d[worst], b, x[worst], M.ulp_distance(got_ord, ref).max()))
    if fn in EXACT:
        assert np.array_equal(bits(got_ord), bits(ref)), key
        keep = ~np.isnan(sref)
        assert np.isnan(got_spec[~keep]).all() and np.array_equal(bits(got_spec[keep]), bits(sref[keep])), (key, sx[keep][got_spec[keep] != sref[keep]])
        return
    assert d[worst] <= b, (key, float(x[worst]), float(got_ord[worst]), float(cr[worst]), d[worst])
    assert M.ulp_distance(got_ord, ref).max() <= b + int(GOLD[key + "/e_ref"]), key
    nan = np.isnan(sref)
    assert np.isnan(got_spec[nan]).all(), (key, sx[nan][~np.isnan(got_spec[nan])])
    fixed = np.isinf(sref) | (sref == 0)
    assert np.array_equal(bits(got_spec[fixed]), bits(sref[fixed])), (key, sx[fixed][got_spec[fixed] != sref[fixed]], got_spec[fixed][got_spec[fixed] != sref[fixed]])
    rest = ~nan & ~fixed
    assert np.isfinite(scr[rest]).all(), key
    ds = M.ulp_distance(got_spec[rest], scr[rest])
    assert ds.max(initial=0) <= b, (key, sx[rest][ds > b], got_spec[rest][ds > b], scr[rest][ds > b])


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c[0] if c[1] is None else "%s@%g" % c)
def test_fixture(dev, case):
    """every function x type x parameter of the fixture, once through the host-pointer form and once through the _dev form"""
    fn, p = case
    for tname in M.TYPES:
        key = M.case_key(fn, p, tname)
        x, sx = GOLD[key + "/ord"][0], GOLD[key + "/spec"][0]
        both = np.concatenate([x, sx])
        param = None if p is None else GOLD[key + "/p"]
        host = dev.math_fn(fn, both, param)
        assert host.dtype == both.dtype
        check_case(fn, host[:x.size], host[x.size:], key)
        t = torch.from_numpy(both).to("cuda:0")
        got = dev.math_fn(fn, t, param)
        assert got.data_ptr() != t.data_ptr() and np.array_equal(bits(t.cpu().numpy()), bits(both))
        device = got.cpu().numpy()
        assert np.array_equal(bits(device), bits(host)), key            # one kernel behind both forms
        check_case(fn, device[:x.size], device[x.size:], key)


# ---------------------------------------------------------------- where the kernel, not the arithmetic, can go wrong
class DevBuf:
    """`nbytes` device bytes at byte offset `off` from a 16-byte boundary, GUARD bytes of FILL on both sides"""

    def __init__(self, nbytes, off=0, data=None):
        host = np.full(GUARD + 16 + nbytes + GUARD, FILL, np.uint8)
        self.at, self.n = GUARD + off, nbytes
        if data is not None:
            host[self.at:self.at + nbytes] = bits(data)
        self.whole = torch.from_numpy(host).to("cuda:0")
        assert self.whole.data_ptr() % 16 == 0
        self.t = self.whole[self.at:self.at + nbytes]

    def result(self, dt):
        """the buffer's bytes, after checking that the guards on both sides are untouched"""
        h = self.whole.cpu().numpy()
        assert (h[:self.at] == FILL).all() and (h[self.at + self.n:] == FILL).all(), "guard bytes written"
        return h[self.at:self.at + self.n].copy().view(dt)


SHAPE_CASES = [("EXP", "float32"), ("LOG", "float64"), ("SQRT", "float32"), ("SQRT", "float64")]
SC = {"float64": 0, "float32": 1}


def shape_sizes(dt):
    per = 16 // np.dtype(dt).itemsize
    return [0, 1, 3, 4, 5, 63, 64, 65, 3 * KBLOCK * per + per + 1]          # the last: three workgroups' worth of units, one more unit and a ragged element


def run_dev(pcx, fn, tname, src, dst, n):
    L = pcx._lib.load()
    pcx._lib.check(L.pcx_mathfn_dev(SC[tname], pcx._lib.MATH_FN[fn], src.data_ptr() if n else None, dst.data_ptr() if n else None, n,
                                    torch.cuda.current_stream().cuda_stream))


@functools.lru_cache(maxsize=None)
def shape_input(fn, tname, n):
    rng = np.random.default_rng(zlib.crc32(("%s/%s/%d" % (fn, tname, n)).encode()))
    return rng.uniform(0.25, 6.0, n).astype(tname)


@pytest.mark.parametrize("fn,tname", SHAPE_CASES)
def test_sizes_and_byte_offsets(pcx, fn, tname):
    """every size at every pair of input and output byte offsets equals the same call on an aligned copy, and writes nothing else"""
    size = np.dtype(tname).itemsize
    for n in shape_sizes(tname):
        x = shape_input(fn, tname, n)
        src, dst = DevBuf(n * size, 0, x), DevBuf(n * size, 0)
        run_dev(pcx, fn, tname, src.t, dst.t, n)
        want = dst.result(tname)
        if n:
            assert np.isfinite(want).all() and not np.array_equal(bits(want), np.full(n * size, FILL, np.uint8))
        for off_in in (0, 4, 8, 12):
            src = DevBuf(n * size, off_in, x)
            for off_out in (0, 4, 8, 12):
                dst = DevBuf(n * size, off_out)
                run_dev(pcx, fn, tname, src.t, dst.t, n)
                assert np.array_equal(bits(dst.result(tname)), bits(want)), (n, off_in, off_out)
            assert np.array_equal(bits(src.result(tname)), bits(x))


@pytest.mark.parametrize("fn,tname", SHAPE_CASES)
def test_out_is_in(pcx, fn, tname):
    size = np.dtype(tname).itemsize
    for n in shape_sizes(tname)[1:]:
        x = shape_input(fn, tname, n)
        src, dst = DevBuf(n * size, 0, x), DevBuf(n * size, 0)
        run_dev(pcx, fn, tname, src.t, dst.t, n)
        for off in (0, 4):
            buf = DevBuf(n * size, off, x)
            run_dev(pcx, fn, tname, buf.t, buf.t, n)
            assert np.array_equal(bits(buf.result(tname)), bits(dst.result(tname))), (n, off)


def test_partial_overlap_is_refused(pcx):
    L, lib = pcx._lib.load(), pcx._lib
    buf = DevBuf(4096, 0, np.ones(1024, np.float32))
    k = np.array([2.0], np.float32)
    p = buf.t.data_ptr()
    for rc in (L.pcx_mathfn_dev(1, lib.MATH_FN["EXP"], p, p + 4, 512, None), L.pcx_mathfn_dev(0, lib.MATH_FN["LOG"], p + 8, p, 256, None),
               L.pcx_mathfn_dev(1, lib.MATH_FN["SQRT"], p, p + 2044, 512, None), L.pcx_mathfn_param_dev(1, lib.MATH_FN["POW"], k.ctypes.data, p + 16, p, 512, None)):
        assert rc == lib.ERR_ARG and "overlaps" in L.pcx_last_error().decode()
    assert L.pcx_mathfn_dev(1, lib.MATH_FN["EXP"], p, p + 2048, 512, None) == lib.OK          # side by side: not an overlap
    torch.cuda.synchronize()
    got = buf.result(np.float32)
    assert (got[:512] == 1).all() and (got[512:] == got[512]).all() and M.ulp_distance(got[512], np.float32(np.e)) <= 1


# ---------------------------------------------------------------- the blocks, through the bundled runner
def make(path, *args, **kw):
    from pothoscomms_amd import blocks as B
    return B.make(path, *args, module="math", **kw)


FIXED_PATHS = {"/comms/exp": "EXP", "/comms/exp2": "EXP2", "/comms/exp10": "EXP10", "/comms/expm1": "EXPM1", "/comms/log": "LOG", "/comms/log2": "LOG2",
               "/comms/log10": "LOG10", "/comms/log1p": "LOG1P", "/comms/sqrt": "SQRT", "/comms/cbrt": "CBRT", "/comms/rsqrt": "RSQRT", "/comms/sinc": "SINC",
               "/comms/sigmoid": "SIGMOID"}
PARAM_PATHS = {"/comms/expN": ("EXPN", 3.0), "/comms/logN": ("LOGN", 3.0), "/comms/pow": ("POW", -1.5), "/comms/nth_root": ("NTH_ROOT", 5.0)}
BLOCK_N = 1001          # elements per work() call: ragged against the 16-byte units of both types
HARD = [-0.0, 0.0, -np.inf, np.inf, np.nan, -8.0, -1.0, 1.0, 8.0, 32.0, -32.0]


def block_input(tname):
    rng = np.random.default_rng(zlib.crc32(tname.encode()))
    x = rng.uniform(0.1, 3.0, BLOCK_N).astype(tname)
    x[:len(HARD)] = HARD
    return x


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a[~np.isnan(a)]), bits(b[~np.isnan(b)]))


@pytest.mark.parametrize("tname", M.TYPES)
def test_one_work_per_path(dev, tname):
    x = block_input(tname)
    for path, fn in FIXED_PATHS.items():
        (out,), consumed, produced = make(path, tname).work_ports([x], BLOCK_N + 5)
        assert consumed == [BLOCK_N] and produced == [BLOCK_N] and same(out, dev.math_fn(fn, x)), path
    for path, (fn, p) in PARAM_PATHS.items():
        (out,), consumed, produced = make(path, tname, p).work_ports([x], BLOCK_N + 5)
        assert consumed == [BLOCK_N] and produced == [BLOCK_N] and same(out, dev.math_fn(fn, x, p)), path
    (out,), consumed, produced = make("/comms/trigonometric", tname, "ATAN").work_ports([x], BLOCK_N + 5)
    assert consumed == [BLOCK_N] and produced == [BLOCK_N] and same(out, dev.math_fn("ATAN", x))


def at(out, v):
    """the output where the input is HARD's v (the sign of a zero counts)"""
    return out[[i for i, h in enumerate(HARD) if np.array([h]).tobytes() == np.array([v]).tobytes()][0]]


def is_zero(v, negative):
    return v == 0 and bool(np.signbit(v)) == negative


@pytest.mark.parametrize("tname", M.TYPES)
def test_setters_land_in_the_expression_the_reference_ends_up_in(dev, tname):
    """Exp.cpp:176-178, Log.cpp:196-198, Root.cpp:247-249: base 2 and root 2 run the generic expression, base 10 and root 3 the special one"""
    x = block_input(tname)
    work = lambda blk: blk.work_ports([x], BLOCK_N)[0][0]
    blk = make("/comms/expN", tname, 7.0)
    for base, (fn, p) in ((2.0, ("EXPN", 2.0)), (10.0, ("EXP10", None)), (0.5, ("EXPN", 0.5))):
        blk.call("setBase", base)
        assert same(work(blk), dev.math_fn(fn, x, p)), base
    blk = make("/comms/logN", tname, 7.0)
    for base, (fn, p) in ((2.0, ("LOGN", 2.0)), (10.0, ("LOG10", None)), (0.5, ("LOGN", 0.5))):
        blk.call("setBase", base)
        out = work(blk)
        assert same(out, dev.math_fn(fn, x, p)), base
        assert np.isnan(at(out, -8.0)) and np.isnan(at(out, -np.inf)) and np.isinf(at(out, 0.0)) and np.isinf(at(out, -0.0))
    blk = make("/comms/nth_root", tname, 7.0)
    for root, (fn, p) in ((2.0, ("NTH_ROOT", 2.0)), (3.0, ("CBRT", None)), (4.0, ("NTH_ROOT", 4.0)), (5.0, ("NTH_ROOT", 5.0)), (-3.0, ("NTH_ROOT", -3.0))):
        blk.call("setRoot", root)
        out = work(blk)
        assert same(out, dev.math_fn(fn, x, p)), root
        if root in (2.0, 4.0):          # pow(x, 1 / root), not sqrt: -0.0 gives +0.0, -inf gives +inf, a negative number a NaN
            assert is_zero(at(out, -0.0), False) and at(out, -np.inf) == np.inf and np.isnan(at(out, -8.0)) and np.isnan(at(out, -32.0))
        elif root == 3.0:               # cbrt: the signs survive
            assert is_zero(at(out, -0.0), True) and at(out, -np.inf) == -np.inf and M.ulp_distance(at(out, -8.0), out.dtype.type(-2)) <= 2
        elif root == 5.0:               # the mirrored power: f = -1 for x < 0, so -0.0 keeps f = 1 and pow gives +0.0
            assert is_zero(at(out, -0.0), False) and at(out, -np.inf) == -np.inf and M.ulp_distance(at(out, -32.0), out.dtype.type(-2)) <= 16
        else:                           # a negative odd root takes the plain power (fmod(-3, 2) is -1): pow(x, -1/3)
            assert at(out, -0.0) == np.inf and is_zero(at(out, -np.inf), False) and np.isnan(at(out, -8.0)) and at(out, 0.0) == np.inf
        assert np.isnan(at(out, np.nan))
    # what sqrt itself does with the same inputs, for contrast
    out = work(make("/comms/sqrt", tname))
    assert is_zero(at(out, -0.0), True) and np.isnan(at(out, -np.inf)) and np.isnan(at(out, -8.0))


def test_dimension_two_counts_as_the_reference_counts(dev):
    """Exp::work hands its loop `elems` (Exp.cpp:136): the first elems SCALARS of 2 * elems are mapped; Root::work multiplies by the
    dimension (Root.cpp:207): all of them are.  Both consume and produce elems elements."""
    n = 777
    x = np.random.default_rng(2).uniform(0.1, 3.0, 2 * n).astype(np.float32)
    (out,), consumed, produced = make("/comms/exp", "float32", dimension=2).work_ports([x], n)
    assert consumed == [n] and produced == [n] and out.size == 2 * n
    assert same(out[:n], dev.math_fn("EXP", x[:n])) and not out[n:].any()
    (out,), consumed, produced = make("/comms/log", "float64", dimension=2).work_ports([x.astype(np.float64)], n)
    assert consumed == [n] and produced == [n] and same(out[:n], dev.math_fn("LOG", x[:n].astype(np.float64))) and not out[n:].any()
    (out,), consumed, produced = make("/comms/sqrt", "float32", dimension=2).work_ports([x], n)
    assert consumed == [n] and produced == [n] and same(out, dev.math_fn("SQRT", x))
    (out,), consumed, produced = make("/comms/pow", "float32", 2.0, dimension=2).work_ports([x], n)
    assert consumed == [n] and produced == [n] and same(out, dev.math_fn("POW", x, 2.0))


def test_set_operation_switches_a_live_block(dev, pcx):
    x = block_input("float32")
    blk = make("/comms/trigonometric", "float32", "COS")
    for op in ("COS", "ACOTH", "SINH", "CSC", "ASEC", "TAN"):
        blk.call("setOperation", op)
        (out,), consumed, produced = blk.work_ports([x], BLOCK_N)
        assert consumed == [BLOCK_N] and same(out, dev.math_fn(op, x)), op
    with pytest.raises(pcx._lib.InvalidArgument, match="Invalid operation"):
        blk.call("setOperation", "VERSINE")
    (out,), _, _ = blk.work_ports([x], BLOCK_N)           # the refused call left the block as it was
    assert same(out, dev.math_fn("TAN", x))
