"""A wider truth for the float FIR plans, and the textbook overlap-save they are measured against (tests/test_fir_truth_cpu.py,
tests/test_fir_truth_gpu.py).  Nothing here needs a GPU.

truth      the reference's polyphase sum (filter/FIRFilter.cpp:286-301) in a wider type: float64 for float32 streams, long double for
           float64 streams, the taps rounded to the stream type first, as the block holds them (floatToQ<QTapsType>, :348).
           Output i is position q = i M + M - 1 of the L-fold stream: y[q] = sum_k h[j + k L] x[K - 1 + n - k], n = q // L, j = q % L.
plain_ols  a textbook overlap-save in the stream's OWN precision on the oracle's transform (oracle.fft, kissfft restated): the stream
           zero-stuffed by L, blocks of N = 4096 doubled until N >= 2 ntaps, forward, times the transform of the taps, inverse, 1 / N,
           every M-th output kept.  It is the reference's arithmetic doing the algorithm the device does: what a sound
           frequency-domain plan costs.
oracle_fir the oracle's own block on the same input: the reference's sequential sum in the stream's precision.

Metrics against the truth t:  l2 = ||got - t||_2 / ||t||_2,  mx = max|got - t| / rms(t).  u is 2^-24 or 2^-53.
Bars: 2 max(E, floor), E the figure of oracle_fir (time-domain plans) or of plain_ols (frequency-domain plans) on the SAME input against
the SAME truth, floor 4 u for l2 and 16 u for mx.  No bar comes from the device's output.
- factor 2: the device takes its radices and its sums in another order, so equal quality is not equal roundings; twice as bad on the
  same input is a defect (the rule of the FFT plans, tests/fft_truth.py).
- floor 4 u: the FFT plans' floor.  Floor 16 u: the largest of up to 10^5 errors whose rms is 4 u lies about four deviations out.
"""
import collections
import functools

import numpy as np

from tests import fir_plans as fp

LD = np.longdouble
CLD = np.clongdouble
LD_EPS = float(np.finfo(LD).eps)
LD_IS_EXTENDED = LD_EPS <= 2e-19            # x87 80-bit or better; where long double is double there is no truth for float64 streams
FLOAT_DTYPES = ("float32", "float64", "complex_float32", "complex_float64")
FLOOR_L2, FLOOR_MX, FACTOR = 4.0, 16.0, 2.0          # in u

FLOAT_ROWS = [r for r in fp.PLANS if r.dtype in FLOAT_DTYPES]


def np_dtype(row):
    return np.float32 if row.dtype.endswith("float32") else np.float64


def unit(row):
    return 2.0 ** -24 if np_dtype(row) == np.float32 else 2.0 ** -53


def is_complex(row):
    return row.dtype.startswith("complex")


def time_domain(row):
    return row.want in ("DIRECT", "EXACT")


def needs_long_double(row):
    return np_dtype(row) == np.float64


def _wide(row):
    return (np.float64, np.complex128) if np_dtype(row) == np.float32 else (LD, CLD)


def as_complex(a, real_t, cplx_t):
    """(n, 2) pairs or a real array -> a complex or real array of the given types, exactly"""
    a = np.asarray(a)
    if a.ndim == 2:
        out = np.empty(a.shape[0], dtype=cplx_t)
        out.real, out.imag = a[:, 0].astype(real_t), a[:, 1].astype(real_t)
        return out
    return a.astype(cplx_t if np.iscomplexobj(a) else real_t)


def rounded_taps(row, taps):
    """the taps as the block holds them: each part rounded to the stream's type; complex when the row's taps are"""
    dt = np_dtype(row)
    t = np.asarray(taps)
    if row.taps == "COMPLEX":
        t = t.astype(np.complex128)
        out = np.empty(t.size, dtype=np.complex64 if dt == np.float32 else np.complex128)
        out.real, out.imag = t.real.astype(dt), t.imag.astype(dt)
        return out
    return np.real(t).astype(dt)


def truth(row, taps, x, n_out):
    """the n_out outputs of the reference's loop over input x (the first K - 1 samples are history), summed in the wide type"""
    real_t, cplx_t = _wide(row)
    L, M, K = row.L, row.M, fp._K(row)
    h = as_complex(rounded_taps(row, taps), real_t, cplx_t)
    xw = as_complex(x, real_t, cplx_t)
    q = np.arange(n_out, dtype=np.int64) * M + (M - 1)
    n, j = q // L, q % L
    out = np.zeros(n_out, dtype=cplx_t if (np.iscomplexobj(h) or np.iscomplexobj(xw)) else real_t)
    for jr in range(L):
        sel = j == jr
        hj = h[jr::L]
        if not sel.any() or hj.size == 0:
            continue
        full = np.convolve(xw, hj)                    # full[K - 1 + n] = sum_k hj[k] x[K - 1 + n - k]
        out[sel] = full[K - 1 + n[sel]]
    return out


def impulse_input(row, x_like, p):
    """zero but a 1 (real part) at iteration p: input index K - 1 + p; the shape and type of the row's own stream"""
    x = np.zeros_like(x_like)
    x[(fp._K(row) - 1 + p,) + ((0,) if x.ndim == 2 else ())] = 1
    return x


def impulse_truth(row, taps, p, n_out):
    """the outputs for impulse_input(p): the rounded taps themselves, y[q] = h[q - p L] where that index exists (exact: 0 + h 1)"""
    real_t, cplx_t = _wide(row)
    h = as_complex(rounded_taps(row, taps), real_t, cplx_t)
    q = np.arange(n_out, dtype=np.int64) * row.M + (row.M - 1)
    i = q - p * row.L
    ok = (i >= 0) & (i < h.size)
    out = np.zeros(n_out, dtype=h.dtype)
    out[ok] = h[i[ok]]
    return out


def oracle_fir(row, taps, x, n_out):
    """the oracle's block on x: complex (or real) in the stream's precision"""
    from oracle import oracle as o
    scalar = o.F32 if np_dtype(row) == np.float32 else o.F64
    blk = o.Fir(scalar, is_complex(row), row.taps == "COMPLEX")
    blk.set_taps(taps); blk.set_decimation(row.M); blk.set_interpolation(row.L); blk.activate()
    y, _, produced, _ = blk.work(x, n_out)
    assert produced == n_out, (row.name, produced, n_out)
    return y


def plain_ols(row, taps, x, n_out):
    """the textbook overlap-save (module docstring), every operation in the stream's precision; (n_out, 2) pairs or a real array"""
    from oracle import oracle as o
    dt = np_dtype(row)
    ct = np.complex64 if dt == np.float32 else np.complex128
    L, M, K = row.L, row.M, fp._K(row)
    h = rounded_taps(row, taps).astype(ct)
    nt = h.size
    N = 4096
    while N < 2 * nt:
        N *= 2
    S = N - (nt - 1)
    xs = as_complex(x, dt, ct).astype(ct)
    G = n_out * M                                   # positions of the L-fold stream the call covers
    # the L-fold stream, history in front: position g of the output is index off + g here; off >= nt - 1 so every block is whole
    off = (K - 1) * L
    lead = max(0, (nt - 1) - off)
    nblocks = -(-G // S)
    v = np.zeros(lead + off + nblocks * S, dtype=ct)
    idx = lead + np.arange(xs.size, dtype=np.int64) * L
    keep = idx < v.size
    v[idx[keep]] = xs[keep]
    start0 = lead + off - (nt - 1)
    frames = np.stack([v[start0 + b * S: start0 + b * S + N] for b in range(nblocks)])
    pairs = lambda a: np.ascontiguousarray(a).view(dt).reshape(-1, 2)
    unpairs = lambda a: np.ascontiguousarray(a).view(ct).reshape(-1)
    hp = np.zeros(N, dtype=ct); hp[:nt] = h
    H = unpairs(o.fft(pairs(hp), N, False))
    X = unpairs(o.fft(pairs(frames.reshape(-1)), N, False)).reshape(nblocks, N)
    Y = (X * H[None, :]).astype(ct)
    y = unpairs(o.fft(pairs(Y.reshape(-1)), N, True)).reshape(nblocks, N) * dt(1.0 / N)
    full = y[:, nt - 1:].reshape(-1)[:G]
    out = np.ascontiguousarray(full[M - 1::M][:n_out].astype(ct))
    assert out.size == n_out, (row.name, out.size, n_out)
    return pairs(out) if is_complex(row) else np.ascontiguousarray(out.real.astype(dt))


# ---- metrics -------------------------------------------------------------------------------------------------------------------
def _diff(row, got, t):
    real_t, cplx_t = _wide(row)
    return as_complex(got, real_t, cplx_t) - t


def l2_mx(row, got, t):
    """(l2, mx) of got against the truth t, both in units of u"""
    d = np.abs(_diff(row, got, t)).astype(np.float64)
    a = np.abs(t).astype(np.float64)
    nrm = float(np.sqrt(np.sum(a ** 2)))
    rms = nrm / np.sqrt(a.size)
    u = unit(row)
    return float(np.sqrt(np.sum(d ** 2))) / nrm / u, float(np.max(d)) / rms / u


def max_abs_err(row, got, t):
    return float(np.max(np.abs(_diff(row, got, t)).astype(np.float64)))


def bars(row, e_ref, e_plain, waived=False):
    """(l2 bar, mx bar) in u from the (l2, mx) pairs of the oracle and of plain_ols; a waived frequency-domain row is held to the
    better-known of the two (PLAIN_BAR_WAIVED of the GPU test)"""
    if time_domain(row):
        e = e_ref
    elif waived:
        e = (max(e_ref[0], e_plain[0]), max(e_ref[1], e_plain[1]))
    else:
        e = e_plain
    return FACTOR * max(e[0], FLOOR_L2), FACTOR * max(e[1], FLOOR_MX)


# the caps that keep the bars meaningful, in u (tests/test_fir_truth_cpu.py asserts them on every float row): the reference's
# sequential sum of K terms grows as about 0.3 sqrt(K) u; a plain overlap-save sits at 3 ... 6 u whatever K is
def ref_caps(K):
    return 1 + np.sqrt(K), 6 * (1 + np.sqrt(K))


PLAIN_CAPS = (16.0, 48.0)

Figures = collections.namedtuple("Figures", "taps x n_in n_out t e_ref e_plain")


@functools.lru_cache(maxsize=None)
def _noise_figures(name):
    from oracle import oracle as o
    row = next(r for r in fp.PLANS if r.name == name)
    taps = fp._taps(row)
    x, n_in, n_out = fp._stream(row, o, o.F32 if np_dtype(row) == np.float32 else o.F64, is_complex(row))
    x.setflags(write=False)
    t = truth(row, taps, x, n_out)
    t.setflags(write=False)
    e_ref = l2_mx(row, oracle_fir(row, taps, x, n_out), t)
    e_plain = l2_mx(row, plain_ols(row, taps, x, n_out), t)
    return Figures(taps, x, n_in, n_out, t, e_ref, e_plain)


def noise_figures(row):
    """the row's own taps and stream, the truth, and the oracle's and plain_ols's (l2, mx) on them: computed once, shared, read-only"""
    return _noise_figures(row.name)


IMPULSES = (0, 1, 4095, 4096)


def impulse_positions(row, n_in):
    """the impulses that fall inside the row's stream (a 64-fold interpolator's stream is a few hundred iterations long)"""
    return [p for p in IMPULSES if fp._K(row) - 1 + p < n_in]


# ---- dynamic range ---------------------------------------------------------------------------------------------------------------
DYN_ITERATIONS = 2 * 4096 + 777
DYN_ROWS = [
    fp.R("dyn cf32 4096-sample 255 taps", "complex_float32", "REAL", 255, plan="CF32_OLS4096"),
    fp.R("dyn cf32 4096-sample 2049 taps", "complex_float32", "REAL", 2049, plan="CF32_OLS4096"),
    fp.R("dyn cf32 partitioned 4097 taps", "complex_float32", "REAL", 4097, plan="CF32_UPOLS"),
    fp.R("dyn cf32 folded M=8 255 taps", "complex_float32", "REAL", 255, M=8, plan="CF32_DECIM"),
    fp.R("dyn cf32 replicated L=4 2049 taps", "complex_float32", "REAL", 2049, L=4, plan="CF32_INTERP"),
    fp.R("dyn f32 real 2049 taps", "float32", "REAL", 2049, plan="F32_OLS4096"),
    fp.R("dyn cf64 2049 taps", "complex_float64", "REAL", 2049, plan="CF64_OLS"),
    fp.R("dyn f64 real 4097 taps", "float64", "REAL", 4097, plan="REAL64_OLS"),
]


def dyn_taps(row):
    """a Blackman-windowed sinc low-pass, real: cut-off 0.05 / max(L, M) cycles per sample at the filter's rate, gain L"""
    n = row.ntaps
    fc = 0.05 / max(row.L, row.M)
    k = np.arange(n) - (n - 1) / 2
    h = 2 * fc * np.sinc(2 * fc * k) * np.blackman(n) if n > 1 else np.ones(1)
    return h / np.sum(h) * row.L


def dyn_stream(row):
    """(x, n_in, n_out): a unit tone in the stop band at 0.31 / L plus one of amplitude 1e-3 in the pass band at 0.01 / max(L, M),
    cycles per input sample; complex exponentials for complex streams, cosines for real ones; rounded to the stream type"""
    K = fp._K(row)
    it = DYN_ITERATIONS
    n_in, n_out = K - 1 + it, (it // row.M) * row.L
    n = np.arange(n_in, dtype=np.float64)
    f_stop, f_pass = 0.31 / row.L, 0.01 / max(row.L, row.M)
    dt = np_dtype(row)
    if is_complex(row):
        z = np.exp(2j * np.pi * f_stop * n) + 1e-3 * np.exp(2j * np.pi * f_pass * n)
        x = np.stack([z.real.astype(dt), z.imag.astype(dt)], axis=1)
    else:
        x = (np.cos(2 * np.pi * f_stop * n) + 1e-3 * np.cos(2 * np.pi * f_pass * n)).astype(dt)
    return np.ascontiguousarray(x), n_in, n_out


def dyn_err(row, got, t, taps, x):
    """max|got - t| / (||h||_1 max|x|) in u"""
    xa = as_complex(x, np.float64, np.complex128)
    scale = float(np.sum(np.abs(rounded_taps(row, taps)).astype(np.float64))) * float(np.max(np.abs(xa)))
    return max_abs_err(row, got, t) / scale / unit(row)


@functools.lru_cache(maxsize=None)
def _dyn_figures(name):
    from oracle import oracle as o
    row = next(r for r in DYN_ROWS if r.name == name)
    taps = dyn_taps(row)
    x, n_in, n_out = dyn_stream(row)
    x.setflags(write=False)
    t = truth(row, taps, x, n_out)
    t.setflags(write=False)
    e_ref = dyn_err(row, oracle_fir(row, taps, x, n_out), t, taps, x)
    e_plain = dyn_err(row, plain_ols(row, taps, x, n_out), t, taps, x)
    return Figures(taps, x, n_in, n_out, t, e_ref, e_plain)


def dyn_figures(row):
    return _dyn_figures(row.name)
