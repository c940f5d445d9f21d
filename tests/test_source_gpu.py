"""GPU suite of /comms/waveform_source and /comms/noise_source (pcx_source_*, device.WaveformSource, device.NoiseSource and the blocks
of libpcx_waveform_blocks.so).

The kernels copy table entries, so everything is held by exact equality: to a numpy walk of arbitrary tables (tests/source_model.py,
which the CPU suite holds to the recorded reference) and to the recorded reference outputs (tests/golden/source.npz).  The one
exception is the SINE table in float64, which the host's libm builds: its documented bound is 1 ulp and it may differ from the libm
that recorded the fixture, so those outputs are held within 1 ulp."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import source_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ES_TYPES = {1: "int8", 2: "int16", 4: "int32", 8: "complex_float32", 16: "complex_float64"}
SIZES = (1, 2, 4096, 1 << 18)
STARTS = (0, 7, (1 << 64) - 5)
OFFSETS = (0, 1, 3)          # elements off a 16-byte boundary
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "source.npz"))


@pytest.fixture(scope="module")
def tables():
    """random bytes for the largest table of the widest element, shared and left unchanged"""
    return np.random.default_rng(46).integers(0, 256, (1 << 18) * 16, dtype=np.uint8)


def steps_of(size):
    return (0, 1, 410, 16, size // 2, (1 << 64) - 1024, 4097)


def lengths_of(tile):
    return (1, 15, 17, tile - 1, tile, tile + 1, 3 * tile + 5)


def run_calls(src, es, lengths, first_offset=0):
    """the calls one after another into one device buffer, each at its own alignment between guard bands; returns [(bytes written
    where the call should have written, ...)] and checks that nothing else was touched"""
    import torch
    spans, pos = [], GUARD
    for k, n in enumerate(lengths):
        pos = (pos + 15) // 16 * 16 + OFFSETS[(k + first_offset) % 3] * es
        spans.append((pos, n * es))
        pos += n * es + GUARD
    buf = torch.full((pos + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    for (at, nbytes), n in zip(spans, lengths):
        src.generate(n, out=base + at)
    host = buf.cpu().numpy()
    outs, mask = [], np.ones(host.size, bool)
    for at, nbytes in spans:
        outs.append(host[at:at + nbytes])
        mask[at:at + nbytes] = False
    assert np.all(host[mask] == FILL), "bytes outside the calls were written"
    return outs


# ---- the kernels against the walk of arbitrary tables
@pytest.mark.parametrize("es", sorted(ES_TYPES))
def test_kernel_equals_the_walk_at_every_size_step_start_length_and_alignment(dev, tables, es):
    src = dev.TableSource(ES_TYPES[es])           # ONE handle: set_table and set_index between calls, the index carried from table to table
    tile = src.geometry()[0]
    assert tile * es == 16 << 10
    index, seen = 0, set()
    for size in SIZES:
        table = tables[:size * es].reshape(size, es)
        for si, step in enumerate(steps_of(size)):
            src.set_table(table, step, entries=size)
            _, period, staged = src.geometry()
            assert period == M.period(size, step) and staged == (max(period * es, 16) <= 8 << 10)
            seen.add(staged)
            # every start with the short lengths and the tile's seams; the long call once per configuration
            for k, start in enumerate(STARTS):
                lengths = lengths_of(tile) if k == si % 3 else lengths_of(tile)[:3] + (tile + 1,)
                if start or k:
                    src.set_index(start)
                    index = start
                assert src.index() == index
                outs = run_calls(src, es, lengths, first_offset=si + k)
                # successive calls continue one walk: together they equal one long call
                want, index = M.walk(table, index, step, sum(lengths))
                assert np.array_equal(np.concatenate(outs), want.reshape(-1)), (es, size, step, start)
                assert src.index() == index
    assert seen == {True, False}
    src.close()


def test_a_host_array_a_tensor_and_a_raw_address_give_the_same_stream(dev, tables):
    import torch
    table = tables[:4096 * 8].reshape(4096, 8)
    outs = []
    for how in ("numpy", "tensor", "address"):
        src = dev.TableSource("complex_float32")
        src.set_table(table, 410, entries=4096)
        src.set_index(123456789)
        n = 5000
        if how == "numpy":
            y = src.generate(n)
        else:
            t = torch.zeros((n, 2), dtype=torch.float32, device="cuda:0")
            src.generate(n, out=t if how == "tensor" else t.data_ptr())
            y = t.cpu().numpy()
        outs.append(y.view(np.uint8).reshape(n, 8))
        assert src.index() == 123456789 + 410 * n
        assert src.generate(0).shape == (0, 2) and src.index() == 123456789 + 410 * n
        src.close()
    want, _ = M.walk(table, 123456789, 410, 5000)
    for y in outs:
        assert np.array_equal(y, want)


GATHER_INNER = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import source_model as M
from pothoscomms_amd import device as dev
rng = np.random.default_rng(47)
out = {}
for es, dt in ((1, "int8"), (4, "int32"), (8, "complex_float32"), (16, "complex_float64")):
    for size, step in ((4096, 410), (1 << 18, 26), (4096, 1), (2, (1 << 64) - 1024)):
        table = rng.integers(0, 256, (size, es), dtype=np.uint8)
        src = dev.TableSource(dt)
        src.set_table(table, step, entries=size)
        src.set_index((1 << 64) - 5)
        n = src.geometry()[0] * 2 + 5
        y = np.concatenate([src.generate(17).view(np.uint8).reshape(-1), src.generate(n).view(np.uint8).reshape(-1)])
        want, index = M.walk(table, (1 << 64) - 5, step, 17 + n)
        assert src.index() == index
        out["%d/%d/%d" % (es, size, step)] = np.array_equal(y, want.reshape(-1))
        src.close()
np.savez(sys.argv[2], **out)
"""


def test_the_diagnostic_gather_gives_the_same_bytes(tmp_path):
    """the per-element gather of libpcx_hip_diag.so (PCX_SRC_GATHER there; the product has no such kernel) on a subset, held to the same walk"""
    diag = os.path.join(ROOT, "pothoscomms_amd", "libpcx_hip_diag.so")
    assert os.path.exists(diag), "make -C pothoscomms_amd/csrc diag"
    res = str(tmp_path / "gather.npz")
    env = dict(os.environ, PCX_HIP_LIBRARY=diag, PCX_SRC_GATHER="1")
    r = subprocess.run([sys.executable, "-c", GATHER_INNER, ROOT, res], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(res)
    assert len(got.files) == 16 and all(bool(got[k]) for k in got.files), {k: bool(got[k]) for k in got.files}


# ---- device.WaveformSource against the recorded reference
def equal_or_one_ulp(got, want, name):
    """exact, but for SINE in float64: within one unit in the last place of the recorded value"""
    if "float64" in name and ("SINE" in name or not name.startswith("matrix/")):
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))), name
    else:
        assert np.array_equal(got, want), name


def test_waveform_source_equals_every_recorded_case(dev, golden):
    for name, dt, wave, ops in M.waveform_cases():
        ampl, offset = M.ampl_offset(dt)
        src, at = None, 0
        out = golden["out/" + name]
        settings = dict(wave=wave, rate=1.0, ampl=complex(*ampl), offset=complex(*offset))
        for op, v in ops:
            if op == "work":
                got = src.generate(v)
                equal_or_one_ulp(got, out[at:at + v], name)
                at += v
            else:
                settings[op] = v
                if src is None:
                    src = dev.WaveformSource(dt, **settings)
                else:
                    src.update(**{op: v})
        assert src.index() == int(golden["state/" + name][-1][3]), name
        src.close()


def test_noise_source_walks_its_table_from_the_drawn_offsets(dev):
    for dt in M.NOISE_TYPES:
        src, twin = dev.NoiseSource(dt, "LAPLACE", mean=0.5, b=0.25, seed=5), dev.NoiseGenerator(5)
        table = twin.table(dt, "LAPLACE", mean=0.5, b=0.25)
        assert np.array_equal(src.table, table)
        index = 0
        for n in (100, 5000, 1):
            got, (want, index) = src.generate(n), M.walk(table, index + twin.next_offset(), 1, n)
            assert np.array_equal(got, want) and src.index() == index
        src.close()


# ---- the blocks through the runner (pcxb_work_ports with no inputs)
def work(b, n):
    outs, consumed, produced = b.work_ports([], [n])
    assert consumed == [] and produced == [n]
    return outs[0]


@pytest.mark.parametrize("path", ["/comms/waveform_source", "/blocks/waveform_source"])
@pytest.mark.parametrize("dt", ["complex_float32", "int16"])
def test_waveform_block_equals_the_fixture(golden, path, dt):
    from pothoscomms_amd import blocks as B
    ampl, offset = M.ampl_offset(dt)
    for wave in M.WAVES:
        b = B.make(path, dt, module="waveform")
        b.call("setWaveform", wave)
        b.call("setAmplitude", complex(*ampl))
        b.call("setOffset", complex(*offset))
        b.call("setFrequency", 0.1)
        b.activate()
        out, at = golden["out/matrix/%s/%s" % (dt, wave)], 0
        for n in M.CALLS:
            assert np.array_equal(work(b, n), out[at:at + n]), (dt, wave, n)
            at += n
        b.call("setDevice", 0)                  # a fresh handle on the device: the settings, the table and the index stay
        assert b.call("getWaveform") == wave and b.call("getFrequency") == 0.1 and b.call("getAmplitude") == complex(*ampl)
        table = golden["table/matrix/%s/%s" % (dt, wave)] if dt in M.FURTHER_TYPES else None
        if table is not None:
            want, _ = M.walk(table, 410 * 600, 410, 77)
            assert np.array_equal(work(b, 77), want)
        b.close()


def test_waveform_block_builds_no_table_before_activate_and_carries_the_index(golden):
    from pothoscomms_amd import _lib, blocks as B
    for dt in M.FURTHER_TYPES:
        b = B.make("/comms/waveform_source", dt, module="waveform")
        ampl, offset = M.ampl_offset(dt)
        b.call("setWaveform", "SINE")
        b.call("setAmplitude", complex(*ampl))
        b.call("setOffset", complex(*offset))
        b.call("setFrequency", 1e-7)            # not achievable: nobody looks before activate()
        with pytest.raises(_lib.PcxError, match="no table"):
            b.work_ports([], [16])
        with pytest.raises(_lib.InvalidArgument, match="step size not achievable"):
            b.activate()
        b.call("setFrequency", 0.1)             # active now: the table follows every setter
        out = golden["out/retune/" + dt]
        got = [work(b, 300)]
        b.call("setFrequency", 1e-4)            # the carried index enters the larger table
        got.append(work(b, 300))
        for g, w in zip(got, (out[:300], out[300:])):
            equal_or_one_ulp(g, w, "retune/" + dt)
        with pytest.raises(_lib.InvalidArgument, match="step size not achievable"):
            b.call("setFrequency", 1e-7)
        with pytest.raises(_lib.InvalidArgument, match="step size not achievable"):
            b.call("setWaveform", "TRIANGLE")       # the refused frequency was kept, and the step is looked at first
        with pytest.raises(_lib.InvalidArgument, match="unknown waveform setting"):
            b.call("setFrequency", 1e-4)            # achievable again: now the wave is looked at
        assert (b.call("getWaveform"), b.call("getFrequency")) == ("TRIANGLE", 1e-4)
        b.call("setWaveform", "SINE")
        assert work(b, 5).shape == M.shape(dt, 5)
        b.close()


def test_noise_block_emits_windows_of_its_table_at_the_drawn_offsets(dev):
    from pothoscomms_amd import blocks as B
    for dt, wave in (("complex_float64", "NORMAL"), ("float32", "LAPLACE"), ("complex_int16", "POISSON"), ("int8", "UNIFORM")):
        k = 100.0 if M.is_integer(dt) else 1.0
        for path in ("/comms/noise_source", "/blocks/noise_source"):
            b = B.make(path, dt, module="waveform")
            b.call("setSeed", M.NOISE_SEED)
            b.call("setWaveform", wave)
            b.call("setMean", M.NOISE_MEAN)
            b.call("setB", M.NOISE_B)
            b.call("setAmplitude", complex(k))
            b.activate()
            twin = dev.NoiseGenerator(M.NOISE_SEED)
            table = twin.table(dt, wave, mean=M.NOISE_MEAN, b=M.NOISE_B, ampl=k)
            index = 0
            for n in (100, 100, 4096 + 5, 1, 100):
                want, index = M.walk(table, index + twin.next_offset(), 1, n)
                assert np.array_equal(work(b, n), want), (dt, wave, n)
            b.call("setDevice", 0)
            assert (b.call("getWaveform"), b.call("getMean"), b.call("getB")) == (wave, M.NOISE_MEAN, M.NOISE_B)
            want, index = M.walk(table, index + twin.next_offset(), 1, 50)
            assert np.array_equal(work(b, 50), want)
            b.call("setB", 0.5)                 # active: a new table from the same generator
            table = twin.table(dt, wave, mean=M.NOISE_MEAN, b=0.5, ampl=k)
            want, index = M.walk(table, index + twin.next_offset(), 1, 50)
            assert np.array_equal(work(b, 50), want)
            b.close()
            twin.close()


def test_the_recorded_noise_windows_through_the_block(golden):
    from pothoscomms_amd import blocks as B
    for name, dt, wave in M.noise_cases():
        b = B.make("/comms/noise_source", dt, module="waveform")
        b.call("setSeed", M.NOISE_SEED)
        b.call("setWaveform", wave)
        b.call("setMean", M.NOISE_MEAN)
        b.call("setB", M.NOISE_B)
        b.call("setAmplitude", complex(100.0 if M.is_integer(dt) else 1.0))
        b.activate()
        out = golden["out/" + name]
        for k, n in enumerate(M.NOISE_CALLS):
            assert np.array_equal(work(b, n), out[100 * k:100 * k + n]), (name, k)
        b.close()


def test_two_noise_blocks_without_a_seed_differ():
    from pothoscomms_amd import blocks as B
    a, b = (B.make("/comms/noise_source", "float64", module="waveform") for _ in range(2))
    a.activate()
    b.activate()
    assert not np.array_equal(work(a, 256), work(b, 256))
    a.close()
    b.close()


def test_a_device_edge_from_the_source_into_rotate(dev, golden, pcx):
    """the source writes the edge's device slab, /comms/rotate reads it: no host buffer on the edge"""
    from pothoscomms_amd import blocks as B
    L = pcx._lib.load()
    src = B.make("/comms/waveform_source", "complex_float32", module="waveform")
    src.call("setWaveform", "SINE")
    src.call("setOffset", 0.25 - 0.5j)
    src.call("setFrequency", 0.1)
    rot = B.make("/comms/rotate", "complex_float32")
    rot.call("setPhase", 0.7)
    src.activate()
    rot.activate()
    n = 600
    edge, kind = src.link_buffer(rot, n * 8)
    assert kind == 2
    k = C.c_int(-1)
    pcx._lib.check(L.pcx_pointer_kind(C.c_void_p(edge), C.byref(k)))
    assert k.value == 2
    yout, pinned = rot.port_buffer(1, (n, 2), np.float32)
    assert src.work_ports_raw([], [], [edge], [n]) == ([], [n])
    assert rot.work_raw(edge, n, yout.ctypes.data, n)[:2] == (n, n)
    want = dev.rotate(golden["out/matrix/complex_float32/SINE"], 0.7)
    assert np.array_equal(yout, want)
    src.close()
    rot.close()


# ---- graphs
def test_a_captured_generate_replays_the_window_it_was_captured_with(dev, tables):
    """what include/pcx.h documents: the carried index is host state, so it moves on by one window when the call is captured and by none
    when the graph is replayed, and every replay writes the captured window"""
    import torch
    table = tables[:4096 * 8].reshape(4096, 8)
    src = dev.TableSource("complex_float32")
    src.set_table(table, 410, entries=4096)
    n = 3 * src.geometry()[0] + 5
    y = torch.zeros((n, 2), dtype=torch.float32, device="cuda:0")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        src.generate(n, out=y, stream=s)                    # the first call, outside the graph: the stream is bound, the period written
    s.synchronize()
    first, index = M.walk(table, 0, 410, n)
    assert np.array_equal(y.cpu().numpy().view(np.uint8).reshape(n, 8), first) and src.index() == index
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        src.generate(n, out=y, stream=s)
    captured, after = M.walk(table, index, 410, n)
    assert src.index() == after
    for _ in range(2):
        y.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy().view(np.uint8).reshape(n, 8), captured)
        assert src.index() == after
    # a call after the replays continues behind the captured window
    nxt, _ = M.walk(table, after, 410, 100)
    assert np.array_equal(src.generate(100).view(np.uint8).reshape(100, 8), nxt)
    src.close()


def test_smoke_chain_the_source_into_freq_demod(dev):
    src = dev.WaveformSource("complex_float32", "SINE", freq=0.1)
    assert src.step == 410 and src.table.shape == (4096, 2)
    x = np.concatenate([src.generate(25000), src.generate(15000)])
    d = dev.FreqDemod("complex_float32").process(x)
    assert np.max(np.abs(d[1:] - 2 * np.pi * 410 / 4096)) <= 1e-5 * np.pi
    whole = dev.WaveformSource("complex_float32", "SINE", freq=0.1)
    assert np.array_equal(whole.generate(40000), x)
