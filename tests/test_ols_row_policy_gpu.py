"""The overlap-save complex_float32 kernels choose a cache policy per stream ROW (ols_block.hpp: a mask of the rows loaded / stored on the
default policy, the others non-temporal).  The masks touch only the full-block fast path, so every case here has a ragged block 0 (the
taps leave pad > 0, or the chain's carried sample), full blocks in the middle and a ragged tail; a policy bit cannot change a value, so
what is checked is that every row still comes from -- and goes to -- where it did.

Sizes: the grid-stride launch at 3 S + 100 outputs (default slots), the dealt launch at 300 S + 100 with a 128-slot share (301 blocks:
more than twice the slots), S = 4096 - overlap.  Bars: 1e-5 of max|ref| against the oracle's FIR (tests/test_parity_gpu.py), 1e-5 pi
against the oracle's Rotate -> FIR -> FreqDemod (tests/test_fullsize_gpu.py).  The oracle's FIR over the whole dealt stream is what this
file costs: 0.1 - 3.4 s a case on one core (n K multiply-adds), about 10 s in all; the references are computed once per (taps, size).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import TOL, ang_err, nerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIR_TAPS = [17, 255, 258, 514, 1026, 2049]      # Kov = 16, 256, 272, 528, 1040, 2048: every rung of the launcher's ladder (<= 256, <= 512, <= 1024, above)
SIZES = {"stride": (None, 3), "dealt": (128, 300)}       # launch path -> (slots, full blocks in front of the 100-sample tail)
GATE_VALUE = 7


def _n_out(overlap, blocks):
    return blocks * (4096 - overlap) + 100


def _fir_overlap(K):
    return (K - 1 + 15) // 16 * 16


def _chain_overlap(K):
    return (K + 31) // 32 * 32          # the FIR's K - 1 and the demodulator's one, in rows of 32


@functools.lru_cache(maxsize=None)
def _fir_case(K, path):
    """(taps, input pairs, the oracle's outputs) -- shared, never written to"""
    from oracle import oracle as o
    from pothoscomms_amd import taps as tp
    n = _n_out(_fir_overlap(K), SIZES[path][1])
    h = tp.complex_bandpass(K, 0.05, 0.05)
    x = np.random.default_rng(1000 * K + n % 997).uniform(-1, 1, (n + K - 1, 2)).astype(np.float32)
    ref = o.Fir(o.F32, True, True); ref.set_taps(h); ref.activate()
    want, c, p, _ = ref.work(x, n)
    assert (c, p) == (n, n)
    x.setflags(write=False); want.setflags(write=False)
    return h, x, want


def _run_fir(dev, h, x, n, slots, gate=None):
    import torch
    from pothoscomms_amd import _lib
    d = torch.device("cuda", 0)
    f = dev.FirFilter("complex_float32", "COMPLEX"); f.set_taps(h); f.set_algo(_lib.FIR_OLS_FFT)
    if slots is not None:
        f.set_slots(slots)
    xd = torch.from_numpy(np.array(x)).to(d)
    y = torch.full((n + 64, 2), float("nan"), dtype=torch.float32, device=d)
    if gate is None:
        assert f.process_dev(xd, y, x.shape[0], n) == (n, n)
    else:
        assert f.process_dev_gated(xd, y, gate, GATE_VALUE, x.shape[0], n) == (n, n, True)
    torch.cuda.synchronize()
    assert f.last_algo == _lib.FIR_OLS_FFT
    out = y.cpu().numpy()
    assert np.isnan(out[n:]).all(), "a store past the produced outputs"
    return out[:n]


@pytest.mark.parametrize("path", sorted(SIZES))
@pytest.mark.parametrize("K", FIR_TAPS)
def test_fir_cf32_rows_against_the_oracle(oracle, dev, K, path):
    h, x, want = _fir_case(K, path)
    got = _run_fir(dev, h, x, want.shape[0], SIZES[path][0])
    err = nerr(got, want)
    print("K=%d %s n=%d nerr=%.3g" % (K, path, want.shape[0], err))
    assert err <= TOL, (K, path, err)


def test_gated_dealt_launch_equals_the_ungated_one(dev):
    import torch
    h, x, want = _fir_case(255, "dealt")
    n = want.shape[0]
    gate = torch.zeros(64, dtype=torch.int32, device=torch.device("cuda", 0))
    gate[0] = GATE_VALUE                    # already open: nothing waits on a later signal
    gated = _run_fir(dev, h, x, n, 128, gate)
    plain = _run_fir(dev, h, x, n, 128)
    assert np.array_equal(gated.view(np.uint32), plain.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _chain_case(K, path):
    from oracle import oracle as o
    from pothoscomms_amd import taps as tp
    n = _n_out(_chain_overlap(K), SIZES[path][1])
    h = tp.c4_taps() if K == 127 else tp.lowpass(K, 0.1)
    assert len(h) == K
    x = np.ascontiguousarray(tp.fm_test_signal(n + K - 1)).view(np.float32).reshape(-1, 2)
    fir = o.Fir(o.F32, True, False); fir.set_taps(h); fir.activate()
    y, c, p, _ = fir.work(o.rotate(x, tp.C4_PHASE), n)
    assert (c, p) == (n, n)
    want = o.FreqDemod(o.F32).work(y)
    x.setflags(write=False); want.setflags(write=False)
    return h, x, want


@pytest.mark.parametrize("path", sorted(SIZES))
@pytest.mark.parametrize("K", [127, 600])
def test_fused_chain_rows_against_the_oracle_chain(oracle, dev, K, path):
    import torch
    from pothoscomms_amd import taps as tp
    h, x, want = _chain_case(K, path)
    n = want.shape[0]
    d = torch.device("cuda", 0)
    ch = dev.FmChain(); ch.set_phase(tp.C4_PHASE); ch.set_taps(h, False); ch.set_slots(128)
    xd = torch.from_numpy(np.array(x)).to(d)
    y = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=d)
    assert ch.process_dev(xd, y, x.shape[0], n) == (n, n)
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    assert np.isnan(out[n:]).all(), "a store past the produced outputs"
    err = ang_err(out[:n], want)
    print("chain K=%d %s n=%d ang_err=%.3g" % (K, path, n, err))
    assert err <= TOL, (K, path, err)


_POLICY_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from pothoscomms_amd import device
from tests.test_ols_row_policy_gpu import _fir_input, _run_fir
h, x, n = _fir_input(255, "dealt")
np.save(%(out)r, _run_fir(device, h, x, n, 128))
print("RESULT ok")
"""


def _fir_input(K, path):
    """the input of _fir_case without the oracle's pass over it"""
    from pothoscomms_amd import taps as tp
    n = _n_out(_fir_overlap(K), SIZES[path][1])
    x = np.random.default_rng(1000 * K + n % 997).uniform(-1, 1, (n + K - 1, 2)).astype(np.float32)
    return tp.complex_bandpass(K, 0.05, 0.05), x, n


def test_product_policy_equals_the_parent_policy_bit_for_bit(dev, tmp_path):
    """one child process under the diagnostic library with the previous row policy switched on (PCX_OLS_NEAR_ROWS=2: two default-policy
    rows at either end of the window), 255 taps, the dealt size: the product library's outputs for the same input are the same bits"""
    diag = os.path.join(ROOT, "pothoscomms_amd", "libpcx_hip_diag.so")
    if not os.path.exists(diag):
        pytest.skip("diagnostic library not built (make -C pothoscomms_amd/csrc diag)")
    out = str(tmp_path / "parent_policy.npy")
    env = dict(os.environ, PCX_HIP_LIBRARY=diag, PCX_OLS_NEAR_ROWS="2")
    r = subprocess.run([sys.executable, "-c", _POLICY_CHILD % {"root": ROOT, "out": out}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, r.stderr[-2000:]
    theirs = np.load(out)
    h, x, n = _fir_input(255, "dealt")
    ours = _run_fir(dev, h, x, n, 128)
    assert np.array_equal(ours.view(np.uint32), theirs.view(np.uint32))
