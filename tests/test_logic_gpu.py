"""GPU tests of the comparator, bitwise, byte-order and const-arithmetic maps (csrc/logic.hip) through the C ABI and through the blocks
of libpcx_logic_blocks.so.  Every result has one right answer: everything is compared with array_equal on the raw bytes, against
tests/golden/logic.npz (what g++ recorded), tests/logic_model.py (numpy's operators, held to the same file by test_logic_cpu.py) and,
for arithmetic with a constant, oracle.arith.

The kernels' geometry, which the sizes below are built around: a lane owns one 16-byte OUTPUT unit, a workgroup of 256 lanes takes
U units per lane and iteration (same-width maps: U = 1 when a lane loads four input units or more for one output unit, else 2; the
comparators of scalars wider than a byte: U = 1, with sizeof(T) input units per output unit), the device grid is one workgroup per
chunk up to 16384, and a call on page-locked host buffers runs on 32 workgroups.
"""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import logic_model as M

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "logic.npz"))
SC = {"float64": 0, "float32": 1, "int64": 2, "int32": 3, "int16": 4, "int8": 5, "uint64": 6, "uint32": 7, "uint16": 8, "uint8": 9}
KBLOCK, HOST_GRID, GUARD, FILL = 256, 32, 64, 0xA5


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def seeded(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def noise(rng, dt, n):
    """n scalars with equal neighbours, zeros and the extremes among them"""
    dt = np.dtype(dt)
    if dt.kind == "f":
        x = rng.integers(-4, 5, n).astype(dt)
        x[rng.integers(0, 8, n) == 0] = np.nan
        x[rng.integers(0, 8, n) == 0] = -0.0
        x[rng.integers(0, 16, n) == 0] = np.inf
        return x
    info = np.iinfo(dt)
    x = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    small = rng.integers(0, 4, n).astype(dt)
    return np.where(rng.integers(0, 2, n) == 0, small, x).astype(dt)


class DevBuf:
    """`nbytes` device bytes at byte offset `off` modulo 16, guard bytes on both sides"""

    def __init__(self, nbytes, off=0, data=None):
        host = np.full(GUARD + 16 + nbytes + GUARD, FILL, np.uint8)
        self.at, self.n = GUARD + off, nbytes
        if data is not None:
            host[self.at:self.at + nbytes] = bits(data)
        self.whole = torch.from_numpy(host).to("cuda:0")
        assert self.whole.data_ptr() % 16 == 0
        self.t = self.whole[self.at:self.at + nbytes]

    def result(self, dt=np.uint8):
        """the buffer's bytes, after checking that the guards on both sides are untouched"""
        h = self.whole.cpu().numpy()
        assert (h[:self.at] == FILL).all() and (h[self.at + self.n:] == FILL).all(), "guard bytes written"
        return h[self.at:self.at + self.n].copy().view(dt)


def units_in_flight(nin, r):
    return 1 if nin * r >= 4 else 2


def compare_units_in_flight(itemsize, nin):
    return 1 if itemsize > 1 else units_in_flight(nin, 1)


def edge_sizes(out_elem, in_elem, nin, r, compare=False):
    """element counts around every path change: the buffer's last unit, the last chunk, counted in output units and in input units"""
    chunk = KBLOCK * (compare_units_in_flight(in_elem, nin) if compare else units_in_flight(nin, r))
    sizes = {0, 1}
    for per_unit in {16 // out_elem, 16 // in_elem}:
        sizes |= {per_unit - 1, per_unit, per_unit + 1, (chunk - 1) * per_unit, chunk * per_unit, (chunk + 1) * per_unit, chunk * per_unit + 1,
                  chunk * per_unit - 1}
    return sorted(s for s in sizes if s >= 0)


CMP_OPS = list(M.CMP)


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("name", M.TYPES)
def test_compare_sizes(dev, name):
    dt = np.dtype(name)
    rng = seeded("cmpsize", name)
    sizes = edge_sizes(1, dt.itemsize, 2, dt.itemsize, compare=True) + edge_sizes(1, dt.itemsize, 1, dt.itemsize, compare=True)
    top = max(sizes)
    a, b = noise(rng, dt, top), noise(rng, dt, top)
    k = a[3]
    for i, n in enumerate(sorted(set(sizes))):
        op = CMP_OPS[i % 6]
        da, db, out = DevBuf(n * dt.itemsize, data=a[:n]), DevBuf(n * dt.itemsize, data=b[:n]), DevBuf(n)
        dev.compare(op, da.t, db.t, scalar=SC[name], out=out.t, n=n)
        assert np.array_equal(out.result(), M.compare(op, a[:n], b[:n])), (op, n)
        out = DevBuf(n)
        dev.compare_const(op, da.t, k, scalar=SC[name], out=out.t, n=n)
        assert np.array_equal(out.result(), M.compare(op, a[:n], k)), (op, n, "const")


SAME_WIDTH = [("not", "uint8"), ("xor2", "uint8"), ("and3", "int16"), ("or2", "uint64"), ("xork", "int32"), ("shl", "int8"), ("shr", "int16"),
              ("shr", "uint32"), ("shr", "int64"), ("swap2", "uint16"), ("swap4", "uint32"), ("swap8", "uint64"), ("X*K", "int16"), ("K/X", "int64"),
              ("X+K", "float32"), ("K-X", "complex64"), ("X/K", "complex128")]


def run_same_width(dev, oracle, kind, name, ins, n, out, k, shift):
    """one call of the map `kind` on device views `ins` of n elements -> (what the model gives for the host arrays)"""
    dt = np.dtype(name)
    cplx = dt.kind == "c"
    sdt = dt if not cplx else np.dtype("float32" if dt == np.complex64 else "float64")
    sc = SC[sdt.name]
    t = [d.t for d in ins]
    if kind == "not":
        dev.bitwise("NOT", t[:1], scalar=sc, out=out, n=n)
    elif kind in ("xor2", "and3", "or2"):
        dev.bitwise(kind[:-1].upper(), t, scalar=sc, out=out, n=n)
    elif kind == "xork":
        dev.bitwise_const("XOR", t[0], k, scalar=sc, out=out, n=n)
    elif kind in ("shl", "shr"):
        dev.bitshift(kind == "shl", t[0], shift, scalar=sc, out=out, n=n)
    elif kind.startswith("swap"):
        dev.byteswap(t[0], width=dt.itemsize, out=out, n=n)
    else:
        dev.arith_const(kind, t[0], k, cplx, scalar=sc, out=out, n=n)


def model_same_width(oracle, kind, name, xs, k, shift):
    dt = np.dtype(name)
    if kind == "not":
        return M.bitwise("NOT", xs[:1])
    if kind in ("xor2", "and3", "or2"):
        return M.bitwise(kind[:-1].upper(), xs)
    if kind == "xork":
        return M.bitwise_const("XOR", xs[0], k)
    if kind in ("shl", "shr"):
        return M.bitshift(kind == "shl", xs[0], shift)
    if kind.startswith("swap"):
        return M.byteswap(xs[0])
    if dt.kind == "c":
        pairs = xs[0].view(xs[0].real.dtype).reshape(-1, 2)
        return M.arith_const(oracle, kind, pairs, np.array([k.real, k.imag], pairs.dtype), True)
    return M.arith_const(oracle, kind, xs[0], k, False)


def same_width_operands(kind, name, n, rng):
    dt = np.dtype(name)
    nin = 3 if kind == "and3" else 2 if kind in ("xor2", "or2") else 1
    if dt.kind == "c":
        xs = [(rng.integers(-50, 51, n) + 1j * rng.integers(1, 60, n)).astype(dt)]
        k = dt.type(3 - 2j)
    elif dt.kind == "f":
        xs = [(rng.standard_normal(n) * 20).astype(dt)]
        k = dt.type(-2.5)
    else:
        xs = [noise(rng, dt, n) for _ in range(nin)]
        k = dt.type(5)
        if kind == "K/X":
            xs[0][xs[0] == -1] = 7          # (MIN beside -1 is test_arith_const_corner_cases')
    return xs, k, 8 * dt.itemsize - 3


@pytest.mark.parametrize("kind,name", SAME_WIDTH)
def test_same_width_sizes(dev, oracle, kind, name):
    dt = np.dtype(name)
    rng = seeded("size", kind, name)
    nin = 3 if kind == "and3" else 2 if kind in ("xor2", "or2") else 1
    sizes = edge_sizes(dt.itemsize, dt.itemsize, nin, 1)
    xs, k, shift = same_width_operands(kind, name, max(sizes), rng)
    for n in sizes:
        ins = [DevBuf(n * dt.itemsize, data=x[:n]) for x in xs]
        out = DevBuf(n * dt.itemsize)
        run_same_width(dev, oracle, kind, name, ins, n, out.t, k, shift)
        want = model_same_width(oracle, kind, name, [x[:n] for x in xs], k, shift) if n else np.zeros(0, dt)
        assert np.array_equal(out.result(), bits(want)), (kind, name, n)


@pytest.mark.parametrize("case", ["cmp/float64", "cmp/uint8", "cmpk/int16", "xor3/uint8", "swap4/uint32", "K/X/int32", "X*K/complex64", "shr/int8"])
def test_three_grid_strides_plus_one_element(dev, oracle, case):
    """calls on page-locked host buffers run on 32 workgroups: three strides of that grid and one element more"""
    kind, name = case.rsplit("/", 1)
    dt = np.dtype(name)
    rng = seeded("stride", case)

    def pinned(x):
        t = torch.empty(max(x.nbytes, 1), dtype=torch.uint8).pin_memory()
        h = t.numpy()[:x.nbytes].view(x.dtype)
        h[...] = x
        return t, h

    if kind in ("cmp", "cmpk"):
        nin = 2 if kind == "cmp" else 1
        n = 3 * HOST_GRID * KBLOCK * compare_units_in_flight(dt.itemsize, nin) * 16 + 1
        (ta, a), (tb, b), (to, o) = pinned(noise(rng, dt, n)), pinned(noise(rng, dt, n)), pinned(np.full(n + 16, FILL, np.uint8))
        if kind == "cmp":
            dev.compare("<=", a, b, out=o[:n])
            want = M.compare("<=", a, b)
        else:
            dev.compare_const("!=", a, 2, out=o[:n])
            want = M.compare("!=", a, 2)
        assert np.array_equal(o[:n], want) and (o[n:] == FILL).all()
        return
    kind3 = {"xor3": "and3"}.get(kind, kind)
    nin = 3 if kind == "xor3" else 1
    n = 3 * HOST_GRID * KBLOCK * units_in_flight(nin, 1) * (16 // dt.itemsize) + 1
    xs, k, shift = same_width_operands(kind3, name, n, rng)
    held = [pinned(x) for x in xs]
    to, o = pinned(np.full((n + 16) * dt.itemsize, FILL, np.uint8))
    out = o[:n * dt.itemsize].view(dt)
    hs = [h for _, h in held]
    if kind == "xor3":
        dev.bitwise("XOR", hs, out=out)
        want = M.bitwise("XOR", xs)
    elif kind == "swap4":
        dev.byteswap(hs[0], out=out)
        want = M.byteswap(xs[0])
    elif kind == "shr":
        dev.bitshift(False, hs[0], shift, out=out)
        want = M.bitshift(False, xs[0], shift)
    else:
        cplx = dt.kind == "c"
        if cplx:
            dev.arith_const(kind, dev.as_pairs(hs[0]), k, True, out=dev.as_pairs(out))
        else:
            dev.arith_const(kind, hs[0], k, False, out=out)
        want = model_same_width(oracle, kind, name, xs, k, shift)
    assert np.array_equal(bits(out), bits(want)) and (o[n * dt.itemsize:] == FILL).all()


# ---------------------------------------------------------------- alignment
def offset_plans(elem, nbuf, rng):
    """every buffer takes every element-aligned offset modulo 16 while the others stay where they are, then some mixed draws"""
    offs = list(range(0, 16, elem))
    base = [offs[(3 * i + 1) % len(offs)] for i in range(nbuf)]
    plans = []
    for i in range(nbuf):
        for o in offs:
            p = list(base)
            p[i] = o
            plans.append(tuple(p))
    plans += [tuple(int(rng.choice(offs)) for _ in range(nbuf)) for _ in range(8)]
    return sorted(set(plans))


@pytest.mark.parametrize("name", ["uint8", "int16", "float32", "float64"])
def test_compare_alignment(dev, name):
    dt = np.dtype(name)
    rng = seeded("cmpalign", name)
    n = KBLOCK * 16 + 3 * 16 + 5                # whole chunks, whole units behind them and a ragged unit
    a, b = noise(rng, dt, n), noise(rng, dt, n)
    plans = sorted({(pa, pb, po) for pa, pb, _ in offset_plans(dt.itemsize, 3, rng) for po in (0, 5)} |
                   {(dt.itemsize % 16, 0, po) for po in range(16)})
    for i, (oa, ob, oo) in enumerate(plans):
        op = CMP_OPS[i % 6]
        da, db, out = DevBuf(a.nbytes, oa, a), DevBuf(b.nbytes, ob, b), DevBuf(n, oo)
        assert out.t.data_ptr() % 16 == oo and da.t.data_ptr() % 16 == oa
        dev.compare(op, da.t, db.t, scalar=SC[name], out=out.t, n=n)
        assert np.array_equal(out.result(), M.compare(op, a, b)), (op, oa, ob, oo)
        out = DevBuf(n, oo)
        dev.compare_const(op, db.t, a[0], scalar=SC[name], out=out.t, n=n)
        assert np.array_equal(out.result(), M.compare(op, b, a[0])), (op, ob, oo, "const")


@pytest.mark.parametrize("kind,name", [("xor2", "uint8"), ("and3", "int16"), ("xork", "int32"), ("shr", "int16"), ("swap2", "uint16"), ("swap8", "uint64"),
                                       ("K/X", "int32"), ("X*K", "complex64"), ("X/K", "float64")])
def test_same_width_alignment(dev, oracle, kind, name):
    dt = np.dtype(name)
    rng = seeded("align", kind, name)
    nin = 3 if kind == "and3" else 2 if kind == "xor2" else 1
    n = (KBLOCK * units_in_flight(nin, 1) + 3) * (16 // dt.itemsize) + (16 // dt.itemsize) // 2
    xs, k, shift = same_width_operands(kind, name, n, rng)
    want = bits(model_same_width(oracle, kind, name, xs, k, shift))
    for plan in offset_plans(dt.itemsize, nin + 1, rng):
        ins = [DevBuf(x.nbytes, o, x) for x, o in zip(xs, plan)]
        out = DevBuf(n * dt.itemsize, plan[-1])
        run_same_width(dev, oracle, kind, name, ins, n, out.t, k, shift)
        assert np.array_equal(out.result(), want), (kind, name, plan)


# ---------------------------------------------------------------- aliasing
@pytest.mark.parametrize("kind,name", [("xor2", "uint8"), ("and3", "int64"), ("not", "int16"), ("xork", "uint32"), ("shl", "int32"), ("swap4", "uint32"),
                                       ("K-X", "int16"), ("X/K", "complex64")])
def test_out_is_an_input(dev, oracle, kind, name):
    dt = np.dtype(name)
    rng = seeded("alias", kind, name)
    nin = 3 if kind == "and3" else 2 if kind == "xor2" else 1
    n = (2 * KBLOCK * 2 + 5) * (16 // dt.itemsize) + 1
    xs, k, shift = same_width_operands(kind, name, n, rng)
    want = bits(model_same_width(oracle, kind, name, xs, k, shift))
    for which in sorted({0, nin - 1}):
        ins = [DevBuf(x.nbytes, 16 % (dt.itemsize * 3) if dt.itemsize < 16 else 0, x) for x in xs]
        run_same_width(dev, oracle, kind, name, ins, n, ins[which].t, k, shift)
        assert np.array_equal(ins[which].result(), want), (kind, name, which)
        for j, (d, x) in enumerate(zip(ins, xs)):
            assert j == which or np.array_equal(d.result(), bits(x))


def test_comparator_out_is_its_one_byte_input(dev):
    rng = seeded("alias", "cmp")
    n = 3 * KBLOCK * 2 * 16 + 7
    for name in ("int8", "uint8"):
        a, b = noise(rng, name, n), noise(rng, name, n)
        for which in (0, 1):
            da, db = DevBuf(n, 3, a), DevBuf(n, 0, b)
            out = (da, db)[which]
            dev.compare(">", da.t, db.t, scalar=SC[name], out=out.t.view(torch.uint8), n=n)
            assert np.array_equal(out.result(), M.compare(">", a, b))
        da = DevBuf(n, 1, a)
        dev.compare_const("<", da.t, 1, scalar=SC[name], out=da.t, n=n)
        assert np.array_equal(da.result(), M.compare("<", a, 1))


def test_partial_overlap_is_refused(dev, pcx):
    n = 4096
    x = np.arange(n, dtype=np.uint8)
    d = DevBuf(2 * n, 0, np.concatenate([x, x]))
    before = d.result().copy()
    InvalidArgument = pcx._lib.InvalidArgument
    with pytest.raises(InvalidArgument):
        dev.bitwise("XOR", [d.t[:n], d.t[n:]], scalar=SC["uint8"], out=d.t[16:16 + n], n=n)
    with pytest.raises(InvalidArgument):
        dev.bitwise("NOT", [d.t[:n]], scalar=SC["uint8"], out=d.t[1:1 + n], n=n)
    with pytest.raises(InvalidArgument):
        dev.bitwise_const("AND", d.t[:n], 3, scalar=SC["uint8"], out=d.t[n - 1:2 * n - 1], n=n)
    with pytest.raises(InvalidArgument):
        dev.bitshift(True, d.t[8:8 + n], 1, scalar=SC["int16"], out=d.t[:n], n=n // 2)
    with pytest.raises(InvalidArgument):
        dev.byteswap(d.t[:n], width=4, out=d.t[4:4 + n], n=n // 4)
    with pytest.raises(InvalidArgument):
        dev.arith_const("X+K", d.t[:n], 1, False, scalar=SC["float32"], out=d.t[64:64 + n], n=n // 4)
    # a comparator of wider scalars may not write into its input at all, not even at its start
    with pytest.raises(InvalidArgument):
        dev.compare(">", d.t[:n], d.t[n:], scalar=SC["float32"], out=d.t[:n // 4], n=n // 4)
    with pytest.raises(InvalidArgument):
        dev.compare_const(">", d.t[:n], 0, scalar=SC["int16"], out=d.t[n - 2:n - 2 + n // 2], n=n // 2)
    with pytest.raises(InvalidArgument):
        dev.compare("==", d.t[:n], d.t[n:], scalar=SC["uint8"], out=d.t[n - 1:2 * n - 1], n=n)
    # the output may be ONE of the inputs: twice among them, a later pass of a long fold would read what an earlier one wrote
    for nin in (2, 3, 9, 17):
        ins = [d.t[n:]] * nin
        ins[0] = ins[-1] = d.t[:n]
        with pytest.raises(InvalidArgument, match="it may be one"):
            dev.bitwise("XOR", ins, scalar=SC["uint8"], out=d.t[:n], n=n)
    torch.cuda.synchronize()
    assert np.array_equal(d.result(), before)


# ---------------------------------------------------------------- N-ary fold
@pytest.mark.parametrize("nin", [2, 3, 8, 9, 17])
@pytest.mark.parametrize("op", ["AND", "OR", "XOR"])
def test_nary_fold(dev, op, nin):
    fn = {"AND": np.bitwise_and, "OR": np.bitwise_or, "XOR": np.bitwise_xor}[op]
    for name in ("uint8", "int64"):
        dt = np.dtype(name)
        rng = seeded("nary", op, nin, name)
        n = (KBLOCK + 3) * (16 // dt.itemsize) + 1
        xs = [noise(rng, dt, n) | dt.type(0x50 if op == "AND" else 0) for _ in range(nin)]
        want = bits(functools.reduce(fn, xs))
        for which in (None, 0, nin - 1):                # a buffer of its own, input 0, the last input
            ins = [DevBuf(x.nbytes, (i * dt.itemsize) % 16, x) for i, x in enumerate(xs)]
            out = DevBuf(n * dt.itemsize, 8) if which is None else ins[which]
            dev.bitwise(op, [d.t for d in ins], scalar=SC[name], out=out.t, n=n)
            assert np.array_equal(out.result(), want), (op, nin, name, which)
        assert np.array_equal(bits(dev.bitwise(op, xs)), want)          # the host form


# ---------------------------------------------------------------- every (type, op) pair against the fixture
def both_forms(call_host, call_dev, ins, out_dt, out_n):
    """the host form on the arrays and the _dev form on device copies of them -> the two results' bytes"""
    host = bits(call_host(*ins))
    dins = [DevBuf(x.nbytes, 0, x) for x in ins]
    out = DevBuf(out_n * np.dtype(out_dt).itemsize)
    call_dev(*[d.t for d in dins], out.t)
    return host, out.result()


@pytest.mark.parametrize("name", M.TYPES)
def test_compare_fixture(dev, name):
    a, b = GOLD["cmp/%s/a" % name], GOLD["cmp/%s/b" % name]
    sc = SC[name]
    for op, key in M.CMP.items():
        want = GOLD["cmp/%s/%s" % (name, key)]
        h, d = both_forms(lambda x, y: dev.compare(op, x, y), lambda x, y, o: dev.compare(op, x, y, scalar=sc, out=o, n=a.size), [a, b], np.uint8, a.size)
        assert np.array_equal(h, want) and np.array_equal(d, want), op
        ci = 0
        while "cmpk/%s/%d/k" % (name, ci) in GOLD.files:
            k = GOLD["cmpk/%s/%d/k" % (name, ci)]
            want = GOLD["cmpk/%s/%d/%s" % (name, ci, key)]
            h, d = both_forms(lambda x: dev.compare_const(op, x, k), lambda x, o: dev.compare_const(op, x, k, scalar=sc, out=o, n=a.size), [a], np.uint8,
                              a.size)
            assert np.array_equal(h, want) and np.array_equal(d, want), (op, ci)
            ci += 1
        assert ci >= 3


@pytest.mark.parametrize("name", M.INT_TYPES)
def test_bitwise_fixture(dev, name):
    a, b, k = GOLD["bit/%s/a" % name], GOLD["bit/%s/b" % name], GOLD["bitk/%s/k" % name]
    sc, n = SC[name], a.size
    h, d = both_forms(lambda x: dev.bitwise("NOT", [x]), lambda x, o: dev.bitwise("NOT", [x], scalar=sc, out=o, n=n), [a], a.dtype, n)
    want = bits(GOLD["bit/%s/NOT" % name])
    assert np.array_equal(h, want) and np.array_equal(d, want)
    for op in ("AND", "OR", "XOR"):
        want = bits(GOLD["bit/%s/%s" % (name, op)])
        h, d = both_forms(lambda x, y: dev.bitwise(op, [x, y]), lambda x, y, o: dev.bitwise(op, [x, y], scalar=sc, out=o, n=n), [a, b], a.dtype, n)
        assert np.array_equal(h, want) and np.array_equal(d, want), op
        want = bits(GOLD["bitk/%s/%s" % (name, op)])
        h, d = both_forms(lambda x: dev.bitwise_const(op, x, k), lambda x, o: dev.bitwise_const(op, x, k, scalar=sc, out=o, n=n), [a], a.dtype, n)
        assert np.array_equal(h, want) and np.array_equal(d, want), (op, "const")


@pytest.mark.parametrize("name", M.INT_TYPES)
def test_every_shift_size_fixture(dev, name):
    a = GOLD["shift/%s/a" % name]
    sc, n = SC[name], a.size
    for left, key in ((True, "L"), (False, "R")):
        rows = GOLD["shift/%s/%s" % (name, key)]
        assert rows.shape == (8 * a.dtype.itemsize, n)
        for s, row in enumerate(rows):
            h, d = both_forms(lambda x: dev.bitshift(left, x, s), lambda x, o: dev.bitshift(left, x, s, scalar=sc, out=o, n=n), [a], a.dtype, n)
            assert np.array_equal(h, bits(row)) and np.array_equal(d, bits(row)), (key, s)


@pytest.mark.parametrize("name", ["uint16", "int16", "uint32", "int32", "float32", "uint64", "int64", "float64", "complex64", "complex128"])
def test_byteswap_fixture(dev, name):
    dt = np.dtype(name)
    w = dt.itemsize if dt.kind != "c" else dt.itemsize // 2
    raw, want = GOLD["swap/%d/a" % w], bits(GOLD["swap/%d/out" % w])
    x = raw[:raw.size // 2 * 2].view(dt) if dt.kind == "c" else raw.view(dt)         # the same bytes read as the type
    want = want[:x.nbytes]
    nsc = x.nbytes // w
    h, d = both_forms(lambda v: dev.byteswap(v), lambda v, o: dev.byteswap(v, width=w, out=o, n=nsc), [x], np.uint8, x.nbytes)
    assert np.array_equal(h, want) and np.array_equal(d, want)
    assert np.array_equal(bits(M.byteswap(x)), want)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", M.TYPES)
def test_arith_const_fixture(dev, name, cplx):
    sc = SC[name]
    for group, ops in (("ak", [(op, "xd" if op == "K/X" else "x", "k") for op in M.ARITHK]),
                       ("ref", [(op, "kbyx_x" if op[0] == "K" else "xbyk_x", "kbyx_k" if op[0] == "K" else "xbyk_k") for op in M.ARITHK])):
        key = "%s/%s/%s" % (group, name, "c" if cplx else "r")
        for op, xkey, kkey in ops:
            x, k, want = GOLD["%s/%s" % (key, xkey)], GOLD["%s/%s" % (key, kkey)], bits(GOLD["%s/%s" % (key, M.ARITHK[op])])
            n = x.shape[0]
            h, d = both_forms(lambda v: dev.arith_const(op, v, k, cplx), lambda v, o: dev.arith_const(op, v, k, cplx, scalar=sc, out=o, n=n), [x], np.uint8,
                              x.nbytes)
            assert np.array_equal(h, want) and np.array_equal(d, want), (group, op)


# ---------------------------------------------------------------- arithmetic with a constant against the oracle
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", M.TYPES)
def test_arith_const_vs_oracle(dev, oracle, name, cplx):
    dt = np.dtype(name)
    rng = seeded("akoracle", name, cplx)
    n = 5000
    shape = (n, 2) if cplx else (n,)
    if dt.kind == "f":
        x, ks = (rng.standard_normal(shape) * 100).astype(dt), (rng.standard_normal((3, 2)) * 10).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
        x[rng.integers(0, 4, shape) == 0] //= dt.type(max(1, info.max // 50))         # small values, zeros among them
        x.reshape(-1)[:4] = [0, 0, 1, info.max]
        ks = np.array([[7, 3], [info.max // 3, 2], [info.max if info.min == 0 else -3, 5]], dt)
    for k in ks:
        k = k if cplx else k[:1]
        for op in M.ARITHK:
            xo = x          # (integers: zeros among the divisors -- the oracle states the result the device gives there)
            want = bits(M.arith_const(oracle, op, xo, k, cplx))
            got = dev.arith_const(op, xo, k, cplx)
            assert np.array_equal(bits(got), want), (op, k)
            d, out = DevBuf(xo.nbytes, dt.itemsize % 16, xo), DevBuf(xo.nbytes, (2 * dt.itemsize) % 16 if not cplx else 0)
            dev.arith_const(op, d.t, k, cplx, scalar=SC[name], out=out.t, n=n)
            assert np.array_equal(out.result(), want), (op, k, "dev")


@pytest.mark.parametrize("name", ["float32", "float64"])
def test_arith_const_passes_a_nan_on(dev, oracle, name):
    """a NaN among the inputs stays a NaN through every operation with a finite constant, and leaves its neighbours alone.  Which
    bits the NaN carries is not compared (the fixture's note: the processors differ there); every other element is, on its bytes"""
    dt = np.dtype(name)
    rng = seeded("aknan", name)
    n = 4099
    x = (rng.standard_normal(n) * 50).astype(dt)
    nan = rng.integers(0, 5, n) == 0
    x[nan] = np.nan
    x[1], x[2] = np.inf, -np.inf
    for op in M.ARITHK:
        want = M.arith_const(oracle, op, x, dt.type(-2.5), False)
        assert np.array_equal(np.isnan(want), nan)
        got = dev.arith_const(op, x, -2.5, False)
        assert np.array_equal(np.isnan(got), nan), op
        assert np.array_equal(bits(got[~nan]), bits(want[~nan])), op


def test_arith_const_corner_cases(dev, oracle):
    """integer x / 0 gives 0 and MIN / -1 gives MIN, as /comms/arithmetic does; K / X with zeros in X"""
    for name in M.INT_TYPES:
        dt = np.dtype(name)
        info = np.iinfo(dt)
        x = np.array([7, info.min, 0, info.max, 5, 0, 1, info.min], dt)
        for k in ([0, 1, 5, info.max] if info.min == 0 else [0, -1, 1, info.min, 5]):
            k = np.array([k], dt)
            for op in ("X/K", "K/X"):
                want = M.arith_const(oracle, op, x, k, False)
                assert np.array_equal(dev.arith_const(op, x, k, False), want), (name, op, k)
        if info.min < 0:
            assert dev.arith_const("X/K", np.array([info.min], dt), -1, False)[0] == info.min
            assert dev.arith_const("K/X", np.array([-1, 0], dt), info.min, False).tolist() == [info.min, 0]


# ---------------------------------------------------------------- the edges of the interface
def test_empty_calls_and_refused_arguments(dev, pcx):
    E = pcx._lib.InvalidArgument
    z8 = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    assert dev.compare(">", z8, z8, scalar=SC["float64"], out=z8, n=0) is z8         # n == 0: no launch, not even the overlap rule
    assert dev.bitwise("XOR", [z8, z8], scalar=SC["uint8"], out=z8, n=0) is z8
    assert dev.byteswap(np.zeros(0, np.uint32)).size == 0
    with pytest.raises(E):
        dev.bitshift(True, z8, 8, scalar=SC["int8"], out=z8, n=64)
    with pytest.raises(E):
        dev.bitshift(False, z8, 64, scalar=SC["uint64"], out=z8, n=8)
    with pytest.raises(E):
        dev.bitwise("AND", [z8], scalar=SC["uint8"], out=z8, n=64)
    with pytest.raises(E):
        dev.bitwise("NOT", [z8, z8], scalar=SC["uint8"], out=z8, n=64)
    with pytest.raises(E):
        dev.bitwise("XOR", [z8, z8], scalar=SC["float32"], out=z8, n=16)
    with pytest.raises(E):
        dev.byteswap(z8, width=1, out=z8, n=64)
    with pytest.raises(E):
        dev.byteswap(z8, width=16, out=z8, n=4)
    L = pcx._lib.load()
    assert L.pcx_compare_dev(SC["uint8"], 6, z8.data_ptr(), z8.data_ptr(), z8.data_ptr(), 64, None) == pcx._lib.ERR_ARG
    assert L.pcx_arith_const_dev(10, 0, 0, z8.data_ptr(), z8.data_ptr(), z8.data_ptr(), 64, None) == pcx._lib.ERR_ARG
    assert L.pcx_arith_const_dev(SC["uint8"], 0, 6, z8.data_ptr(), z8.data_ptr(), z8.data_ptr(), 64, None) == pcx._lib.ERR_ARG
    torch.cuda.synchronize()
    assert not z8.any().item()


# ---------------------------------------------------------------- the blocks of libpcx_logic_blocks.so
def make(path, dtype, *args, dimension=1):
    from pothoscomms_amd import blocks as B
    return B.make(path, dtype, *args, dimension=dimension, module="logic")


def stream(rng, dtype, nscalars):
    """nscalars scalars of a Pothos type name as the array blocks.py takes: complex as (n, 2) pairs"""
    cplx = dtype.startswith("complex_")
    dt = np.dtype(dtype[8:] if cplx else dtype)
    if dt.kind == "f":
        x = (rng.standard_normal(nscalars * (2 if cplx else 1)) * 30).astype(dt)
    else:
        x = noise(rng, dt, nscalars * (2 if cplx else 1))
    return x.reshape(-1, 2) if cplx else x


BLOCK_N = 1000          # elements per work() call: ragged against the 16-byte units of every type and dimension used here


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("name", ["int8", "int16", "int32", "int64", "float32", "float64"])
def test_comparator_block(name, dim):
    rng = seeded("blk/cmp", name, dim)
    a, b = noise(rng, name, BLOCK_N * dim), noise(rng, name, BLOCK_N * dim)
    for op in M.CMP:
        blk = make("/comms/comparator", name, op, dimension=dim)
        (out,), consumed, produced = blk.work_ports([a, b], BLOCK_N + 7)
        # the reference compares elems * (the OUTPUT's dimension, 1) scalars and consumes elems elements: Comparator.cpp:169
        assert consumed == [BLOCK_N, BLOCK_N] and produced == [BLOCK_N] and out.dtype == np.int8
        assert np.array_equal(out.view(np.uint8), M.compare(op, a[:BLOCK_N], b[:BLOCK_N])), op


def test_comparator_dimension_quirk_at_two():
    """inputs of dimension 2: the first `elems` SCALARS of the buffers are compared, `elems` elements (2 * elems scalars) consumed"""
    rng = seeded("blk/quirk")
    n = 777
    a, b = noise(rng, "int16", 2 * n), noise(rng, "int16", 2 * n)
    blk = make("/comms/comparator", "int16", "<", dimension=2)
    (out,), consumed, produced = blk.work_ports([a, b], n)
    assert consumed == [n, n] and produced == [n] and out.size == n
    assert np.array_equal(out.view(np.uint8), M.compare("<", a[:n], b[:n]))
    assert not np.array_equal(out.view(np.uint8), M.compare("<", a[0::2][:n], b[0::2][:n]))        # (not one scalar per element)
    blk = make("/comms/const_comparator", "float32", ">=", dimension=2)
    blk.call("setConstant", 1.0)
    x = noise(rng, "float32", 2 * n)
    out, consumed, produced, _, _ = blk.work(x, n)
    assert (consumed, produced) == (n, n) and np.array_equal(out.view(np.uint8), M.compare(">=", x[:n], np.float32(1.0)))


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("name", M.TYPES)
def test_const_comparator_block(name, dim):
    rng = seeded("blk/cmpk", name, dim)
    x = noise(rng, name, BLOCK_N * dim)
    blk = make("/comms/const_comparator", name, "!=", dimension=dim)
    out, consumed, produced, _, _ = blk.work(x, BLOCK_N)
    assert (consumed, produced) == (BLOCK_N, BLOCK_N) and np.array_equal(out.view(np.uint8), M.compare("!=", x[:BLOCK_N], 0))     # the default constant
    k = x[5] if not np.isnan(x[5]) else x.dtype.type(2)
    blk.call("setConstant", k.item())
    assert blk.call("constant") == k.item()
    out, consumed, produced, _, _ = blk.work(x, BLOCK_N)            # the second call sees the new constant
    assert np.array_equal(out.view(np.uint8), M.compare("!=", x[:BLOCK_N], k))


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("name", M.TYPES)
def test_const_arithmetic_block(oracle, name, cplx, dim):
    rng = seeded("blk/ak", name, cplx, dim)
    dtype = ("complex_" if cplx else "") + name
    x = stream(rng, dtype, BLOCK_N * dim)
    dt = np.dtype(name)
    if dt.kind == "f":
        k1, k2 = (2.5 - 0.5j, -1.25 + 3j) if cplx else (2.5, -0.75)
    else:
        k1, k2 = (3 + 2j, 5 + 1j) if cplx else (np.int64(3), np.int64(7))
    for op in M.ARITHK:
        blk = make("/comms/const_arithmetic", dtype, op, k1, dimension=dim)
        sink = make("/comms/const_arithmetic", dtype, "X+K", k1)
        blk.connect_signal("constantChanged", sink, "setConstant")
        for k in (k1, k2):
            if k is k2:
                blk.call("setConstant", k)
                assert sink.call("constant") == blk.call("constant") == (k if cplx or dt.kind == "f" else int(k))      # the signal carries the value
            out, consumed, produced, _, _ = blk.work(x, BLOCK_N)
            kk = np.array([k.real, k.imag], dt) if cplx else np.array([k], dt)
            assert (consumed, produced) == (BLOCK_N, BLOCK_N)
            assert np.array_equal(bits(out), bits(M.arith_const(oracle, op, x, kk, cplx))), (op, k)


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("name", M.INT_TYPES)
def test_bitwise_blocks(name, dim):
    rng = seeded("blk/bit", name, dim)
    dt = np.dtype(name)
    n = BLOCK_N * dim
    xs = [noise(rng, name, n) for _ in range(5)]
    blk = make("/comms/bitwise_unary", name, "NOT", dimension=dim)
    out, consumed, produced, _, _ = blk.work(xs[0], BLOCK_N + 3)
    assert (consumed, produced) == (BLOCK_N, BLOCK_N) and np.array_equal(out, M.bitwise("NOT", xs[:1]))
    for op in ("AND", "OR", "XOR"):
        for nch in (2, 5):
            blk = make("/comms/bitwise_binary", name, op, nch, dimension=dim)
            (out,), consumed, produced = blk.work_ports(xs[:nch], BLOCK_N)
            assert consumed == [BLOCK_N] * nch and produced == [BLOCK_N] and np.array_equal(out, M.bitwise(op, xs[:nch])), (op, nch)
        k1, k2 = xs[1][0], xs[1][1]
        blk = make("/comms/const_bitwise_binary", name, k1, op, dimension=dim)
        out, _, _, _, _ = blk.work(xs[0], BLOCK_N)
        assert np.array_equal(out, M.bitwise_const(op, xs[0], k1)), op
        blk.call("setConstant", int(k2))
        assert blk.call("constant") == int(k2)
        out, _, _, _, _ = blk.work(xs[0], BLOCK_N)
        assert np.array_equal(out, M.bitwise_const(op, xs[0], k2)), (op, "after setConstant")
    for left, opname in ((True, "LEFTSHIFT"), (False, "RIGHTSHIFT")):
        blk = make("/comms/bitshift", name, opname, 1, dimension=dim)
        seen = make("/comms/bitshift", "uint64", "LEFTSHIFT", 0)
        blk.connect_signal("shiftSizeChanged", seen, "setShiftSize")
        out, consumed, produced, _, _ = blk.work(xs[2], BLOCK_N)
        assert (consumed, produced) == (BLOCK_N, BLOCK_N) and np.array_equal(out, M.bitshift(left, xs[2], 1))
        s = 8 * dt.itemsize - 1
        blk.call("setShiftSize", s)
        assert seen.call("shiftSize") == s
        out, _, _, _, _ = blk.work(xs[2], BLOCK_N)
        assert np.array_equal(out, M.bitshift(left, xs[2], s))


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("dtype", ["int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64", "complex_int16", "complex_uint32",
                                   "complex_uint16", "complex_int32", "complex_int64", "complex_uint64", "complex_float32", "complex_float64"])
def test_byte_order_block(dtype, dim):
    rng = seeded("blk/swap", dtype, dim)
    x = stream(rng, dtype, BLOCK_N * dim)
    blk = make("/comms/byte_order", dtype, dimension=dim)
    out, consumed, produced, _, _ = blk.work(x, BLOCK_N + 1)
    assert (consumed, produced) == (BLOCK_N, BLOCK_N) and np.array_equal(bits(out), bits(x.byteswap()))      # "Swap Order" by default
    for order, swaps in (("Little Endian", False), ("Big Endian", True), ("Network to Host", True), ("Host to Network", True)):
        blk.call("setByteOrder", order)
        out, consumed, produced, _, _ = blk.work(x, BLOCK_N // 2)         # the output's room bounds the call
        want = x.byteswap() if swaps else x
        assert (consumed, produced) == (BLOCK_N // 2, BLOCK_N // 2)
        assert np.array_equal(bits(out), bits(want)[:out.nbytes]), order
