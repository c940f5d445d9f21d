"""GPU tests of the special-function maps (csrc/specfn.hip) -- gamma, lngamma, erf, erfc, beta, modf -- through the C ABI, host and
device forms, and through the blocks of libpcx_special_blocks.so.

THE BARS, in units in the last place against `cr`, the correctly rounded value of the exact expression
(tests/golden/specfn.npz, mpmath), as specfn_model.ulp_distance measures them.
  * MODF, both outputs, both types: the recorded bits wherever the recorded value is not a NaN, a NaN wherever it is one.
  * float32 GAMMA, LNGAMMA, ERF, ERFC, BETA: the double expression rounded once -- within 1 unit of cr, within 1 + e_ref of ref.
  * float64 GAMMA, ERF, ERFC: 16, the double-precision bound of the OpenCL C specification's table of built-in accuracy for tgamma,
    erf and erfc -- QUOTED FROM MEMORY, as DESIGN.md 20's figures are; no copy of the table was at hand.
  * float64 LNGAMMA: that table leaves lgamma undefined; 16 is a CEILING, the figure the same table gives the same library's tgamma.
    The inputs are well-conditioned (the reference's own e_ref on them is 2).  What the device library does is in
    profiles/specfn/accuracy.md.
  * float64 BETA: the per-input bound of specfn_model.beta_bound, derived there from the expression with L = 16.
  * special inputs: a NaN where ref is a NaN (payloads are not compared), the same value with the same sign where ref is an infinity
    or a zero, the ordinary bar elsewhere.

THE LARGE ARGUMENTS OF BETA.  Term by term the expression loses its value once the larger argument is large: lgamma(1e10) and
lgamma(1e10 + 1) are 2.2e11, a unit in the last place of which is 3.05e-5, and their difference carries that error into the exponent
-- beta(1e10, 1) came out 1.0000025e-10 on float32, 36 units from cr, where the bar is 1.  From 1024 on csrc/specfn.hip therefore takes
the difference of the two log-gammas from Stirling's series, whose leading terms cancel in closed form.  The group "large" of the
fixture (the larger argument from just below 1024 to 1e12, either order) holds that path and its seam to the same bars: float32
within 1 unit of cr, float64 within the per-input bound of the expression.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import specfn_model as S

pytestmark = pytest.mark.gpu

GOLD = np.load(S.GOLD_PATH)
BAR64 = {"GAMMA": 16, "LNGAMMA": 16, "ERF": 16, "ERFC": 16}
KBLOCK, GUARD, FILL = 256, 64, 0xA5
SC = {"float64": 0, "float32": 1}


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a[~np.isnan(a)]), bits(b[~np.isnan(b)]))


def bars(fn, dt, ins):
    """the bar of every input of one case, in units of dt"""
    n = ins[0].size
    if dt == np.float32:
        return np.ones(n)
    if fn == "BETA":
        return S.beta_bounds(ins[0], ins[1], np.float64)
    return np.full(n, BAR64[fn], dtype=np.float64)


def check_exact(got, ref, what):
    keep = ~np.isnan(ref)
    assert np.isnan(got[~keep]).all(), what
    assert np.array_equal(bits(got[keep]), bits(ref[keep])), (what, got[keep][got[keep] != ref[keep]], ref[keep][got[keep] != ref[keep]])


def check_case(fn, tname, got_ord, got_spec):
    """hold one case's results on the ordinary and the special inputs to the bars above; prints the largest distances first"""
    key = S.case_key(fn, tname)
    ord_, spec = GOLD[key + "/ord"], GOLD[key + "/spec"]
    nin = 2 if fn == "BETA" else 1
    x, ref, cr = ord_[:nin], ord_[nin], ord_[nin + 1]
    sx, sref, scr = spec[:nin], spec[nin], spec[nin + 1]
    b = bars(fn, x.dtype.type, x)
    d = S.ulp_distance(got_ord, cr)
    worst = int(np.argmax(d / b))
    print("%-16s ordinary: largest distance from the truth %g (bar %g) at %r; from the reference %g" % (key, d.max(), b[worst], x[:, worst].tolist(), S.ulp_distance(got_ord, ref).max()))
    assert (d <= b).all(), (key, x[:, worst].tolist(), float(got_ord[worst]), float(cr[worst]), d[worst], b[worst])
    assert (S.ulp_distance(got_ord, ref) <= b + int(GOLD[key + "/e_ref"])).all(), key
    nan = np.isnan(sref)
    assert np.isnan(got_spec[nan]).all(), (key, sx[:, nan][:, ~np.isnan(got_spec[nan])], got_spec[nan][~np.isnan(got_spec[nan])])
    fixed = np.isinf(sref) | (sref == 0)
    wrong = bits(got_spec[fixed]).reshape(-1, x.dtype.itemsize) != bits(sref[fixed]).reshape(-1, x.dtype.itemsize)
    assert not wrong.any(), (key, sx[:, fixed][:, wrong.any(axis=1)], got_spec[fixed][wrong.any(axis=1)], sref[fixed][wrong.any(axis=1)])
    rest = ~nan & ~fixed
    assert np.isfinite(scr[rest]).all(), key
    ds, bs = S.ulp_distance(got_spec[rest], scr[rest]), bars(fn, x.dtype.type, sx[:, rest])
    print("%-16s special:  largest distance from the truth %g, distances over the bar %r" % (key, ds.max(initial=0), list(zip(sx[:, rest][:, ds > bs].T.tolist(), ds[ds > bs]))))
    assert (ds <= bs).all(), (key, sx[:, rest][:, ds > bs], got_spec[rest][ds > bs], scr[rest][ds > bs], ds[ds > bs])


def call(dev, fn, *xs):
    """one function of the family on numpy arrays (the host form) or device tensors (the _dev form); modf -> (int, frac)"""
    if fn == "BETA":
        return dev.beta(*xs)
    if fn == "MODF":
        return dev.modf(*xs)
    return dev.special_fn(fn, *xs)


@pytest.mark.parametrize("tname", S.TYPES)
@pytest.mark.parametrize("fn", S.FUNCS)
def test_fixture(dev, fn, tname):
    """every function x type of the fixture, once through the host-pointer form and once through the _dev form: equal bits, both held
    to the bars"""
    key = S.case_key(fn, tname)
    nin = 2 if fn == "BETA" else 1
    n_ord = GOLD[key + "/ord"].shape[1]
    both = [np.concatenate([GOLD[key + "/ord"][k], GOLD[key + "/spec"][k]]) for k in range(nin)]
    host = call(dev, fn, *both)
    ts = [torch.from_numpy(a).to("cuda:0") for a in both]
    got = call(dev, fn, *ts)
    for t, a in zip(ts, both):
        assert np.array_equal(bits(t.cpu().numpy()), bits(a))               # the inputs are left as they were
    if fn == "MODF":
        for part, h, g in zip((1, 2), host, got):
            assert h.dtype == both[0].dtype and g.data_ptr() != ts[0].data_ptr()
            g = g.cpu().numpy()
            assert np.array_equal(bits(g), bits(h)), (key, part)            # one kernel behind both forms
            check_exact(g, np.concatenate([GOLD[key + "/ord"][part], GOLD[key + "/spec"][part]]), (key, part))
        return
    assert host.dtype == both[0].dtype and all(got.data_ptr() != t.data_ptr() for t in ts)
    device = got.cpu().numpy()
    assert np.array_equal(bits(device), bits(host)), key                    # one kernel behind both forms
    check_case(fn, tname, host[:n_ord], host[n_ord:])
    check_case(fn, tname, device[:n_ord], device[n_ord:])


@pytest.mark.parametrize("tname", S.TYPES)
def test_beta_large_arguments(dev, tname):
    """the larger argument from just below 1024, where the evaluation changes, to 1e12: host and device forms, equal bits, the bars of beta"""
    a, b, ref, cr = GOLD["BETA/%s/large" % tname]
    host = dev.beta(a, b)
    device = dev.beta(torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")).cpu().numpy()
    assert np.array_equal(bits(device), bits(host))
    d, bar = S.ulp_distance(host, cr), bars("BETA", a.dtype.type, np.stack([a, b]))
    worst = int(np.argmax(d / bar))
    print("BETA/%s large: largest distance from the truth %g (bar %g) at (%r, %r); the reference's %g" % (tname, d.max(), bar[worst], a[worst], b[worst], S.ulp_distance(ref, cr).max()))
    assert (d <= bar).all(), (a[d > bar], b[d > bar], host[d > bar], cr[d > bar], d[d > bar])


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


SHAPE_CASES = [("ERF", "float32"), ("LNGAMMA", "float64"), ("BETA", "float32"), ("BETA", "float64"), ("MODF", "float32"), ("MODF", "float64")]
OFFSETS = (0, 4, 12)


def shape_sizes(dt):
    per = 16 // np.dtype(dt).itemsize
    return [0, 1, 3, 4, 5, 63, 64, 65, 3 * KBLOCK * per + per + 1]          # the last: three workgroups' worth of units, one more unit and a ragged element


def n_in(fn):
    return 2 if fn == "BETA" else 1


def n_out(fn):
    return 2 if fn == "MODF" else 1


def run_dev(pcx, fn, tname, srcs, dsts, n):
    """the _dev call on device addresses (None for every pointer when n is 0: nothing may be touched)"""
    L, lib = pcx._lib.load(), pcx._lib
    ptr = lambda p: p if n else None
    st = torch.cuda.current_stream().cuda_stream
    if fn == "BETA":
        lib.check(L.pcx_beta_dev(SC[tname], ptr(srcs[0]), ptr(srcs[1]), ptr(dsts[0]), n, st))
    elif fn == "MODF":
        lib.check(L.pcx_modf_dev(SC[tname], ptr(srcs[0]), ptr(dsts[0]), ptr(dsts[1]), n, st))
    else:
        lib.check(L.pcx_specfn_dev(SC[tname], lib.SPEC_FN[fn], ptr(srcs[0]), ptr(dsts[0]), n, st))


@functools.lru_cache(maxsize=None)
def shape_input(fn, tname, n, which=0):
    rng = np.random.default_rng(zlib.crc32(("%s/%s/%d/%d" % (fn, tname, n, which)).encode()))
    return rng.uniform(0.25, 6.0, n).astype(tname)


@functools.lru_cache(maxsize=None)
def aligned_result(pcx, fn, tname, n):
    """the call on buffers at offset 0: what every other placement must equal, computed once and shared"""
    size = np.dtype(tname).itemsize
    srcs = [DevBuf(n * size, 0, shape_input(fn, tname, n, k)) for k in range(n_in(fn))]
    dsts = [DevBuf(n * size, 0) for _ in range(n_out(fn))]
    run_dev(pcx, fn, tname, [s.t.data_ptr() for s in srcs], [d.t.data_ptr() for d in dsts], n)
    want = [d.result(tname) for d in dsts]
    for w in want:
        w.setflags(write=False)
        if n:
            assert np.isfinite(w).all() and not np.array_equal(bits(w), np.full(n * size, FILL, np.uint8))
    return want


@pytest.mark.parametrize("fn,tname", SHAPE_CASES)
def test_sizes_and_byte_offsets(pcx, fn, tname):
    """every size with every buffer at byte offset 0, 4 or 12 independently equals the same call on aligned buffers, and writes nothing else"""
    size = np.dtype(tname).itemsize
    nbuf = n_in(fn) + n_out(fn)
    for n in shape_sizes(tname):
        want = aligned_result(pcx, fn, tname, n)
        xs = [shape_input(fn, tname, n, k) for k in range(n_in(fn))]
        for combo in np.ndindex(*([len(OFFSETS)] * nbuf)):
            offs = [OFFSETS[i] for i in combo]
            srcs = [DevBuf(n * size, o, x) for o, x in zip(offs, xs)]
            dsts = [DevBuf(n * size, o) for o in offs[n_in(fn):]]
            run_dev(pcx, fn, tname, [s.t.data_ptr() for s in srcs], [d.t.data_ptr() for d in dsts], n)
            for d, w in zip(dsts, want):
                assert np.array_equal(bits(d.result(tname)), bits(w)), (n, offs)
            for s, x in zip(srcs, xs):
                assert np.array_equal(bits(s.result(tname)), bits(x)), (n, offs)


@pytest.mark.parametrize("fn,tname", SHAPE_CASES)
def test_aliasing(pcx, fn, tname):
    """out exactly in (unary), out exactly in0 or in1 and in0 identical to in1 (beta), out_int or out_frac exactly in (modf)"""
    size = np.dtype(tname).itemsize
    for n in shape_sizes(tname)[1:]:
        want = aligned_result(pcx, fn, tname, n)
        xs = [shape_input(fn, tname, n, k) for k in range(n_in(fn))]
        for off in (0, 4):
            if fn == "BETA":
                for k in (0, 1):                    # out is input k
                    bufs = [DevBuf(n * size, off, x) for x in xs]
                    run_dev(pcx, fn, tname, [b.t.data_ptr() for b in bufs], [bufs[k].t.data_ptr()], n)
                    assert np.array_equal(bits(bufs[k].result(tname)), bits(want[0])), (n, off, k)
                    assert np.array_equal(bits(bufs[1 - k].result(tname)), bits(xs[1 - k]))
                # one buffer as both inputs, and as the output too: beta(x, x)
                buf, dst = DevBuf(n * size, off, xs[0]), DevBuf(n * size, 0)
                run_dev(pcx, fn, tname, [buf.t.data_ptr()] * 2, [dst.t.data_ptr()], n)
                twice = dst.result(tname)
                run_dev(pcx, fn, tname, [buf.t.data_ptr()] * 2, [buf.t.data_ptr()], n)
                assert np.array_equal(bits(buf.result(tname)), bits(twice)) and not np.array_equal(bits(twice), bits(want[0]))
            elif fn == "MODF":
                for k in (0, 1):                    # output k is the input
                    buf, other = DevBuf(n * size, off, xs[0]), DevBuf(n * size, off)
                    dsts = [buf, other] if k == 0 else [other, buf]
                    run_dev(pcx, fn, tname, [buf.t.data_ptr()], [d.t.data_ptr() for d in dsts], n)
                    for d, w in zip(dsts, want):
                        assert np.array_equal(bits(d.result(tname)), bits(w)), (n, off, k)
            else:
                buf = DevBuf(n * size, off, xs[0])
                run_dev(pcx, fn, tname, [buf.t.data_ptr()], [buf.t.data_ptr()], n)
                assert np.array_equal(bits(buf.result(tname)), bits(want[0])), (n, off)


def test_overlaps_are_refused_and_neighbours_accepted(pcx):
    import math
    L, lib = pcx._lib.load(), pcx._lib
    x = np.full(6 * 256, 2.5, np.float32)           # six quarters Q0 ... Q5 of 256 elements, 1024 bytes each
    buf = DevBuf(x.nbytes, 0, x)
    p = buf.t.data_ptr()
    Q = [p + 1024 * k for k in range(6)]
    F = lib.SPEC_FN
    refused = [L.pcx_specfn_dev(1, F["ERF"], p, p + 4, 512, None), L.pcx_specfn_dev(0, F["LNGAMMA"], p + 8, p, 256, None),
               L.pcx_specfn_dev(1, F["GAMMA"], p, p + 2044, 512, None),
               L.pcx_beta_dev(1, p, p + 2048, p + 4, 256, None), L.pcx_beta_dev(1, p, p + 2048, p + 2044, 256, None),
               L.pcx_beta_dev(0, p + 8, p + 2048, p, 128, None), L.pcx_beta_dev(1, p, p + 4, p, 256, None),          # out is in0 and cuts into in1
               L.pcx_modf_dev(1, p, p + 4, p + 2048, 256, None), L.pcx_modf_dev(1, p, p + 2048, p + 1020, 256, None),
               L.pcx_modf_dev(1, p, p + 1024, p + 1024, 256, None), L.pcx_modf_dev(1, p, p + 1024, p + 1028, 256, None),  # the outputs on each other
               L.pcx_modf_dev(1, p, p, p, 256, None)]
    for rc in refused:
        assert rc == lib.ERR_ARG and "overlaps" in L.pcx_last_error().decode(), (rc, L.pcx_last_error())
    torch.cuda.synchronize()
    assert np.array_equal(buf.result(np.float32), x)                        # nothing was queued
    # side by side is not an overlap: erf of Q0 into Q1, beta of Q0 and Q5 into Q2, modf of Q0 into Q3 and Q4
    assert L.pcx_specfn_dev(1, F["ERF"], Q[0], Q[1], 256, None) == lib.OK
    assert L.pcx_beta_dev(1, Q[0], Q[5], Q[2], 256, None) == lib.OK
    assert L.pcx_modf_dev(1, Q[0], Q[3], Q[4], 256, None) == lib.OK
    assert L.pcx_beta_dev(1, Q[0], Q[0] + 4, Q[5], 255, None) == lib.OK     # inputs that overlap each other are only read
    torch.cuda.synchronize()
    got = buf.result(np.float32).reshape(6, 256)
    assert (got[0] == 2.5).all() and (got[3] == 2).all() and (got[4] == 0.5).all()
    assert (got[1] == got[1, 0]).all() and S.ulp_distance(got[1, 0], np.float32(math.erf(2.5))) <= 1
    assert (got[2] == got[2, 0]).all() and S.ulp_distance(got[2, 0], np.float32(math.gamma(2.5) ** 2 / 24)) <= 1      # gamma(2.5)^2 / gamma(5)
    assert (got[5, :255] == got[2, 0]).all() and got[5, 255] == 2.5


# ---------------------------------------------------------------- the blocks, through the bundled runner
def make(path, *args, **kw):
    from pothoscomms_amd import blocks as B
    return B.make(path, *args, module="special", **kw)


UNARY_PATHS = {"/comms/gamma": "GAMMA", "/comms/lngamma": "LNGAMMA", "/comms/erf": "ERF", "/comms/erfc": "ERFC"}
BLOCK_N = 1001          # elements per work() call: ragged against the 16-byte units of both types
HARD = [-0.0, 0.0, -np.inf, np.inf, np.nan, -1.0, 1.0, -8.0, 8.0, -2.5]


def block_input(tname, n=BLOCK_N, seed=0):
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (tname, seed)).encode()))
    x = rng.uniform(0.1, 3.0, n).astype(tname)
    x[:len(HARD)] = HARD
    return x


@pytest.mark.parametrize("tname", S.TYPES)
def test_one_work_per_path(dev, tname):
    x = block_input(tname)
    for path, fn in UNARY_PATHS.items():
        (out,), consumed, produced = make(path, tname).work_ports([x], BLOCK_N + 5)
        assert consumed == [BLOCK_N] and produced == [BLOCK_N] and same(out, dev.special_fn(fn, x)), path
    # beta takes the shorter of its inputs, whichever port it is on
    longer = block_input(tname, BLOCK_N + 40, seed=1)
    for ins, left in (([x, longer], [BLOCK_N, BLOCK_N]), ([longer, x], [BLOCK_N, BLOCK_N])):
        (out,), consumed, produced = make("/comms/beta", tname).work_ports(ins, BLOCK_N + 60)
        assert consumed == left and produced == [BLOCK_N] and same(out, dev.beta(ins[0][:BLOCK_N], ins[1][:BLOCK_N]))
    # modf's two named ports; the room of the smaller output decides
    blk = make("/comms/modf", tname)
    assert [p[0] for p in blk.ports(1)] == ["int", "frac"]
    (ip, fp), consumed, produced = blk.work_ports([x], [BLOCK_N + 5, BLOCK_N + 9])
    want_i, want_f = dev.modf(x)
    assert consumed == [BLOCK_N] and produced == [BLOCK_N, BLOCK_N] and same(ip, want_i) and same(fp, want_f)
    (ip, fp), consumed, produced = blk.work_ports([x], [BLOCK_N - 7, BLOCK_N])
    assert consumed == [BLOCK_N - 7] and produced == [BLOCK_N - 7] * 2 and same(ip, want_i[:BLOCK_N - 7]) and same(fp, want_f[:BLOCK_N - 7])


def test_dimension_two_maps_every_scalar(dev):
    """all four work() functions multiply by the dimension (Gamma.cpp:77, ErrorFunction.cpp:80, Beta.cpp:71, ModF.cpp:82): 2 * elems
    scalars are mapped, elems elements consumed and produced"""
    n = 777
    x = np.random.default_rng(2).uniform(0.1, 3.0, 2 * n).astype(np.float32)
    y = np.random.default_rng(3).uniform(0.1, 3.0, 2 * n).astype(np.float32)
    for path, fn in UNARY_PATHS.items():
        for tname in S.TYPES:
            (out,), consumed, produced = make(path, tname, dimension=2).work_ports([x.astype(tname)], n)
            assert consumed == [n] and produced == [n] and out.size == 2 * n and same(out, dev.special_fn(fn, x.astype(tname))), (path, tname)
    (out,), consumed, produced = make("/comms/beta", "float32", dimension=2).work_ports([x, y], n)
    assert consumed == [n, n] and produced == [n] and out.size == 2 * n and same(out, dev.beta(x, y))
    (ip, fp), consumed, produced = make("/comms/modf", "float64", dimension=2).work_ports([x.astype(np.float64)], n)
    want_i, want_f = dev.modf(x.astype(np.float64))
    assert consumed == [n] and produced == [n, n] and ip.size == 2 * n and same(ip, want_i) and same(fp, want_f)
