"""/comms/iir_filter restated: the sequential double recurrence the device is held to, its narrowing, the Schur-Cohn
test and the SCAN bound of pcx_iir_set_taps, a small bilinear-transform designer for the filters the tests name, and a residual check
for streams too long for the model.

The recurrence, per component, in this order (the SERIAL plan computes exactly this, the SCAN plan within the bound):
    v = b_0 x[n];  v = v + b_k x[n-k], k = 1..N
    w = a_1 y[n-1];  w = w + a_k y[n-k], k = 2..N
    y[n] = v - w                       (y[n] = v for N = 0)
with b, a divided by a_0 in double, the history zero after create / reset / set_taps, and y narrowed per component: float32 to
nearest, float64 as is, integers toward zero, saturated at the range of the type, NaN -> 0."""
import math

import numpy as np

SCALARS = {"float64": np.float64, "float32": np.float32, "int64": np.int64, "int32": np.int32, "int16": np.int16, "int8": np.int8}
DEFAULT_TAPS = [0.0676, 0.135, 0.0676, 1, -1.142, 0.412]
U = 2.0 ** -53


def split(dtype):
    return (dtype[len("complex_"):], True) if dtype.startswith("complex_") else (dtype, False)


def normalise(taps):
    t = np.asarray(taps, np.float64)
    n1 = t.shape[0] // 2
    a0 = t[n1]
    b, a = t[:n1] / a0, t[n1:] / a0
    a[0] = 1.0
    return b, a


def narrow(y, name):
    """y: float64 array -> the element type"""
    y = np.asarray(y, np.float64)
    if name == "float64":
        return y.copy()
    if name == "float32":
        return y.astype(np.float32)
    t = SCALARS[name]
    info = np.iinfo(t)
    with np.errstate(invalid="ignore"):
        hi = 2.0 ** 63 if name == "int64" else float(info.max)
        lo = -2.0 ** 63 if name == "int64" else float(info.min)
        out = np.zeros(y.shape, t)
        ok = np.isfinite(y) & (y < hi) & (y > lo)
        out[ok] = np.trunc(y[ok]).astype(t)
        out[~np.isnan(y) & (y >= hi)] = info.max
        out[~np.isnan(y) & (y <= lo)] = info.min
    return out


class Model:
    """the sequential recurrence with its carried history; process(x) takes (n,) or (n, 2) element arrays"""

    def __init__(self, taps=DEFAULT_TAPS, cplx=False):
        self.b, self.a = (list(map(float, v)) for v in normalise(taps))
        self.N = len(self.b) - 1
        self.C = 2 if cplx else 1
        self.reset()

    def reset(self):
        self.xh = [[0.0] * self.N for _ in range(self.C)]      # xh[c][k-1] = x[n-k]
        self.yh = [[0.0] * self.N for _ in range(self.C)]

    def process_double(self, x):
        x = np.asarray(x)
        xs = x.reshape(x.shape[0], -1).astype(np.float64)
        out = np.zeros(xs.shape, np.float64)
        b, a, N = self.b, self.a, self.N
        for c in range(self.C):
            xh, yh = self.xh[c], self.yh[c]
            col = xs[:, c].tolist()
            res = [0.0] * len(col)
            for n, xn in enumerate(col):
                v = b[0] * xn
                for k in range(1, N + 1):
                    v = v + b[k] * xh[k - 1]
                if N >= 1:
                    w = a[1] * yh[0]
                    for k in range(2, N + 1):
                        w = w + a[k] * yh[k - 1]
                    y = v - w
                else:
                    y = v
                if N:
                    xh.insert(0, xn)
                    xh.pop()
                    yh.insert(0, y)
                    yh.pop()
                res[n] = y
            out[:, c] = res
        return out.reshape(x.shape)

    def process(self, x, name):
        return narrow(self.process_double(x), name)


def run(x, taps, name):
    """(double outputs, narrowed outputs) from a zero history; name: the scalar type"""
    cplx = np.asarray(x).ndim == 2
    yd = Model(taps, cplx).process_double(x)
    return yd, narrow(yd, name)


# ---- the plan and the bound of pcx_iir_set_taps (pcx_iir_api.hip iir_configure)
def schur_cohn(a):
    """reflection coefficients of a (a[0] = 1) by the step-down recursion; None when one of them is not inside the unit circle"""
    a = [float(v) for v in a]
    ks = []
    for m in range(len(a) - 1, 0, -1):
        k = a[m]
        if not abs(k) < 1.0:
            return None
        ks.append(k)
        d = 1.0 - k * k
        a = [(a[i] - k * a[m - i]) / d for i in range(m)]
    return ks


def impulse_l1(num, a, nmax=1 << 20):
    """(l1 norm, peak) of num/a's impulse response once it has decayed (the last max(N, 1) samples below 2^-60 of the sum), else None"""
    N = len(a) - 1
    y = np.zeros(nmax)
    s = pk = 0.0
    a = [float(v) for v in a]
    for n in range(nmax):
        v = float(num[n]) if n < len(num) else 0.0
        for k in range(1, min(N, n) + 1):
            v -= a[k] * y[n - k]
        y[n] = v
        s += abs(v)
        pk = max(pk, abs(v))
        if not math.isfinite(s):
            return None
        if n >= len(num) + N and n >= 64 and max(abs(y[n - k]) for k in range(max(N, 1))) <= s * 2.0 ** -60:
            return s, pk
    return None


def plan(taps):
    """("SCAN", bound) or ("SERIAL", 0.0), as the handle computes them"""
    b, a = normalise(taps)
    N = len(a) - 1
    if schur_cohn(a) is None:
        return "SERIAL", 0.0
    ra, rh = impulse_l1([1.0], a), impulse_l1(b, a)
    if ra is None or rh is None:
        return "SERIAL", 0.0
    S, hA = ra
    NB = 2
    while NB < N:
        NB *= 2
    M = np.zeros((NB, NB))
    M[0, :N] = -a[1:]
    M[np.arange(1, NB), np.arange(NB - 1)] = 1.0
    P = np.linalg.matrix_power(M, 16)
    K = 1.0
    for d in range(9):
        K = max(K, np.abs(P).sum(1).max())
        if d < 8:
            P = P @ P
    rho = np.abs(P).sum(1).max()
    Q = np.linalg.matrix_power(P, 64)
    for d in range(8):
        K = max(K, np.abs(Q).sum(1).max())
        Q = Q @ Q
    B, Aa = np.abs(b).sum(), np.abs(a[1:]).sum()
    Z = S * B
    Kh = max(1.0, Aa * hA)
    w, r = 0.0, 1.0
    for _ in range(64):
        w += r
        r = min(1.0, r * rho)
    levels = 8 + 1 + 1 + 2 * w + 8
    bound = U * S * (N + 1) * (2 * B + Aa * Z) + U * levels * (NB + 1) * (K + 1) * Z * Kh
    return ("SCAN", float(bound)) if math.isfinite(bound) else ("SERIAL", 0.0)


# ---- a bilinear-transform designer (scipy.signal's butter / cheby1 for low-pass, restated); wn: cut-off / Nyquist
def _zpk_lowpass(z, p, k, wn):
    fs = 2.0
    warped = 2 * fs * math.tan(math.pi * wn / fs)
    z, p = z * warped, p * warped
    k = k * warped ** (len(p) - len(z))
    fs2 = 2 * fs
    zd = (fs2 + z) / (fs2 - z)
    pd = (fs2 + p) / (fs2 - p)
    zd = np.append(zd, -np.ones(len(pd) - len(zd)))
    kd = k * np.real(np.prod(fs2 - z) / np.prod(fs2 - p))
    return np.real(kd * np.poly(zd)), np.real(np.poly(pd))


def butter(order, wn):
    m = np.arange(-order + 1, order, 2)
    p = -np.exp(1j * np.pi * m / (2 * order))
    return _zpk_lowpass(np.array([]), p, 1.0, wn)


def cheby1(order, rp, wn):
    eps = math.sqrt(10 ** (0.1 * rp) - 1.0)
    mu = 1.0 / order * math.asinh(1 / eps)
    m = np.arange(-order + 1, order, 2)
    p = -np.sinh(mu + 1j * np.pi * m / (2 * order))
    k = np.real(np.prod(-p))
    if order % 2 == 0:
        k = k / math.sqrt(1 + eps * eps)
    return _zpk_lowpass(np.array([]), p, k, wn)


def taps_of(ba):
    b, a = ba
    return list(np.concatenate([b, a]))


def named_set():
    """the filters whose SCAN bound the issue pins at 1e-10 (cut-offs in cycles per sample: wn = 2 f)"""
    return {"default": list(DEFAULT_TAPS), "butter2_0.01": taps_of(butter(2, 0.02)), "butter4_0.1": taps_of(butter(4, 0.2)),
            "butter6_0.2": taps_of(butter(6, 0.4)), "cheby1_4_0.1dB_0.2": taps_of(cheby1(4, 0.1, 0.4))}


# ---- orders 9 to 32: the SCAN buckets NB = 16 and 32, and every one of the 32 carried history slots
SPREAD_ORDERS = (9, 12, 16, 17, 24, 31, 32)
COMBS = ((9, 0.5), (16, -0.5), (17, -0.9), (31, 0.5), (32, -0.5))
UNSTABLE_ORDERS = (3, 9, 16, 17, 31, 32)


def _draw(seed, N):
    """(pole-pair angles, b of l1 norm 1 and every |b_k| >= 0.01) of order N, drawn in this order"""
    rng = np.random.default_rng(seed)
    k = N // 2
    ang = (np.arange(k) + 0.5 + rng.uniform(-0.2, 0.2, k)) * np.pi / k
    b = rng.uniform(0.2, 1, N + 1) * rng.choice([-1, 1], N + 1)
    return ang, b / np.abs(b).sum()


def spread(N, last_radius=None):
    """order N with its pole pairs spread over the upper half circle at radii 0.7 ... 0.9 (a real pole at 0.5 for an odd N) and
    every feedforward tap of weight; last_radius moves the last pair"""
    ang, b = _draw(N, N)
    k = N // 2
    rad = np.linspace(0.7, 0.9, k)
    if last_radius is not None:
        rad[-1] = last_radius
    p = rad * np.exp(1j * ang)
    poles = np.concatenate([p, np.conj(p), [0.5] if N % 2 else []])
    a = np.real(np.poly(poles))
    return list(np.concatenate([b, a]))


def comb(N, g):
    """a = 1 + g z^-N: the whole feedback on the oldest history slot of the order (b drawn behind the angles, as spread's is)"""
    a = np.zeros(N + 1)
    a[0], a[N] = 1.0, g
    return list(np.concatenate([_draw(100 + N, N)[1], a]))


def high_order_set():
    """spreadN and combN plan as SCAN with a bound below 1e-10, unstableN (a pole pair at radius 1.004) as SERIAL"""
    s = {"spread%d" % N: spread(N) for N in SPREAD_ORDERS}
    s.update({"comb%d" % N: comb(N, g) for N, g in COMBS})
    s.update({"unstable%d" % N: spread(N, 1.004) for N in UNSTABLE_ORDERS})
    return s


# ---- the residual check (numpy or torch float64 arrays)
def residual_check(x, y, taps, name, bound, xmax=None, skip=0):
    """first index n >= skip (-1: none) where r[n] = y[n] + sum a_k y[n-k] - sum b_k x[n-k] leaves its tolerance.  x, y: float64 arrays of
    (n,) or (n, C), a zero history in front; y the narrowed outputs, widened.  Each output differs from the exact recurrence by its
    narrowing (< 1 for integers, half an ulp of float32) plus twice bound * max|x| (the plan's bound, and the model's own error,
    which is the first term of that bound); the residual is evaluated in double, with its own rounding on top."""
    torch = None
    if type(x).__module__.startswith("torch"):
        import torch
    b, a = normalise(taps)
    N = len(a) - 1
    n = x.shape[0]
    if xmax is None:
        xmax = float(abs(x).max())
    if name.startswith("int"):
        q = abs(y) * 0 + 1.0
    elif name == "float32":
        q = abs(y) * 2.0 ** -24
    else:
        q = abs(y) * 0
    e = q + 2.0 * bound * xmax
    r = y * 1.0
    tol = e * 1.0
    mag = abs(y) * 1.0
    for k in range(1, N + 1):
        r[k:] = r[k:] + float(a[k]) * y[:n - k]
        tol[k:] = tol[k:] + abs(float(a[k])) * e[:n - k]
        mag[k:] = mag[k:] + abs(float(a[k])) * abs(y[:n - k])
    for k in range(0, N + 1):
        r[k:] = r[k:] - float(b[k]) * x[:n - k]
        mag[k:] = mag[k:] + abs(float(b[k])) * abs(x[:n - k])
    tol = tol + 4 * (2 * N + 2) * U * mag
    bad = abs(r) > tol
    if r.ndim == 2:
        bad = bad.any(1)
    bad[:skip] = False
    if torch is not None:
        idx = torch.nonzero(bad)
        return int(idx[0, 0]) if idx.numel() else -1
    idx = np.flatnonzero(bad)
    return int(idx[0]) if idx.size else -1
