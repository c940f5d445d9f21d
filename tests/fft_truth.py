"""A plain higher-precision truth for the FFT plans (tests/test_fft_plans_gpu.py, tests/test_fft_truth_cpu.py).

The device's float32 plans are held to numpy's float64 transform (truth64: its error is about 2e-16 against 6e-8), the float64 plans
to a long-double transform written here (truth_ld: 1.1e-19 against 1.1e-16).  Every twiddle of truth_ld comes from an index reduced in
integers -- (k * n) % N, and n * n % (2 N) for the chirp -- and from an angle inside the first quadrant, so no phase loses digits
to its size.  Frames are rows: every function takes (n, 2) pairs or a complex array of whole frames and returns (nframes, nbins).

Conventions are the device's (include/pcx.h): forward exp(-j ...), inverse exp(+j ...), neither scaled.
"""
import functools

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
LD_EPS = float(np.finfo(LD).eps)
LD_IS_EXTENDED = LD_EPS <= 2e-19            # x87 80-bit or better; where long double is double, truth_ld is no truth for float64
LD_LIMIT = 1 << 17                          # truth_ld is used up to this many bins
_HALF_PI = LD("1.57079632679489661923132169163975144209858469968755")


def frames(x, nbins):
    """(n, 2) pairs or a complex array -> complex (nframes, nbins), in the precision of x"""
    a = np.asarray(x)
    if not np.iscomplexobj(a):
        a = a.reshape(-1, 2)
        a = a[:, 0] + 1j * a[:, 1] if a.dtype != LD else a[:, 0] + CLD(1j) * a[:, 1]
    return a.reshape(-1, nbins)


def cis(j, n):
    """exp(-2 pi i j / n) in long double for an integer array j, every j reduced modulo n first: the angle handed to cos / sin lies in
    [0, pi / 2), the quadrant is applied exactly"""
    j = np.asarray(j, dtype=np.int64) % n
    q, r = np.divmod(4 * j, n)
    a = _HALF_PI * r.astype(LD) / LD(n)
    c, s = np.cos(a), np.sin(a)
    re = np.choose(q, [c, -s, -c, s])
    im = np.choose(q, [-s, -c, s, c])
    out = np.empty(j.shape, dtype=CLD)
    out.real, out.imag = re, im
    return out


@functools.lru_cache(maxsize=2)
def _table(n):
    """exp(-2 pi i j / n), j = 0 ... n - 1.  Where 8 divides n only the first octant goes through cos / sin: the rest are its mirror
    images, exactly (the large sizes are all of this kind, and the libm calls are what a table costs)."""
    if n % 8 == 0:
        e, q = n // 8, n // 4
        o = cis(np.arange(e + 1, dtype=np.int64), n)
        c = np.concatenate([o.real, -o.imag[e - 1::-1]])[:q]          # cos over the first quadrant: cos(pi/2 - a) = sin(a)
        s = np.concatenate([-o.imag, o.real[e - 1::-1]])[:q]          # sin over it
        t = np.empty(n, dtype=CLD)
        t.real = np.concatenate([c, -s, -c, s])
        t.imag = np.concatenate([-s, -c, s, c])
    else:
        t = cis(np.arange(n, dtype=np.int64), n)
    t.setflags(write=False)
    return t


def truth64(x, nbins, inverse=False):
    """numpy's float64 transform of every frame: the truth for complex_float32"""
    a = frames(x, nbins).astype(np.complex128)
    return np.fft.ifft(a, axis=1) * nbins if inverse else np.fft.fft(a, axis=1)


def _radix2(a, inverse):
    """vectorised decimation-in-time radix 2 over the last axis (a power of two), long double"""
    nf, n = a.shape
    if n == 1:
        return a.copy()
    bits = n.bit_length() - 1
    idx = np.arange(n, dtype=np.int64)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    a = a[:, rev]
    tab = _table(n)
    half = 1
    while half < n:
        w = tab[np.arange(half, dtype=np.int64) * (n // (2 * half))]
        if inverse:
            w = np.conj(w)
        v = a.reshape(nf, n // (2 * half), 2, half)
        lo, hi = v[:, :, 0, :], v[:, :, 1, :] * w
        a = np.stack([lo + hi, lo - hi], axis=2).reshape(nf, n)
        half *= 2
    return a


def truth_ld(x, nbins, inverse=False):
    """the long-double transform of every frame: the truth for complex_float64.  Powers of two by radix 2; any other size by
    chirp-z over it (X[k] = w[k] sum_n x[n] w[n] conj(w[k - n]), w[n] = exp(-j pi n^2 / N) with n^2 reduced modulo 2 N)."""
    assert nbins <= LD_LIMIT, nbins
    a = frames(x, nbins).astype(CLD)
    if nbins & (nbins - 1) == 0:
        return _radix2(a, inverse)
    if inverse:                      # the inverse kernel is the conjugate of the forward one
        a = np.conj(a)
    n = np.arange(nbins, dtype=np.int64)
    w = cis((n * n) % (2 * nbins), 2 * nbins)
    m = 1
    while m < 2 * nbins - 1:
        m *= 2
    u = np.zeros((a.shape[0], m), dtype=CLD)
    u[:, :nbins] = a * w
    b = np.zeros((1, m), dtype=CLD)
    b[0, :nbins] = np.conj(w)
    b[0, m - nbins + 1:] = np.conj(w[1:][::-1])
    conv = _radix2(_radix2(u, False) * _radix2(b, False), True) / LD(m)
    out = conv[:, :nbins] * w
    return np.conj(out) if inverse else out


def direct_ld(x, nbins, inverse=False):
    """the O(N^2) long-double DFT, every twiddle from (k * n) % N: what truth_ld is checked against"""
    a = frames(x, nbins).astype(CLD)
    k = np.arange(nbins, dtype=np.int64)
    out = np.empty_like(a)
    for i in range(nbins):
        w = _table(nbins)[(k * i) % nbins]
        out[:, i] = np.sum(a * (np.conj(w) if inverse else w), axis=1)
    return out


def impulse_truth(nbins, p, inverse=False):
    """the transform of a unit impulse at sample p: bin k is the bare twiddle exp(-+ 2 pi i p k / N)"""
    k = np.arange(nbins, dtype=np.int64)
    t = _table(nbins)[(k * int(p)) % nbins]
    return np.conj(t) if inverse else t


def tone(nbins, k, dtype, inverse=False):
    """(x, truth): the unit tone exp(+2 pi i k n / N) rounded to dtype as (nbins, 2) pairs, and the transform of that rounded input --
    the line N at bin k (forward) or -k mod N (inverse), plus the transform of the rounding residue.  The residue is 2^-24 or 2^-53 of
    the signal, so numpy's float64 transform of it is exact to 1e-16 of that."""
    n = np.arange(nbins, dtype=np.int64)
    ideal = np.conj(_table(nbins)[(n * int(k)) % nbins])
    x = np.stack([ideal.real.astype(dtype), ideal.imag.astype(dtype)], axis=1)
    resid = ((x[:, 0].astype(LD) - ideal.real) + CLD(1j) * (x[:, 1].astype(LD) - ideal.imag)).astype(np.complex128)
    truth = (np.fft.ifft(resid) * nbins if inverse else np.fft.fft(resid)).astype(CLD)
    truth[(-int(k)) % nbins if inverse else int(k) % nbins] += LD(nbins)
    return x, truth


# ---- the bars ------------------------------------------------------------------------------------------------------------------
UNIT = {"complex_float32": 2.0 ** -24, "complex_float64": 2.0 ** -53}      # u: the unit roundoff of the device type


def bar(e_ref, u, factor=2):
    """factor * max(E_ref, 4 u): E_ref is the oracle's own error on the same input against the same truth.  The device takes its
    radices in another order, so equal quality is not equal roundings (factor 2); kissfft is nearly exact at 2 ... 8 bins (floor 4 u)."""
    return factor * max(float(e_ref), 4 * u)


def oracle_cap(nbins, u):
    """what the oracle's own error may be before a bar built on it means nothing: u (4 ceil(log2 N) + p), p the largest prime
    factor where kissfft has no butterfly of its own for it (p > 5), else 0.  A radix-2 ... 5 stage is a twiddle product and a short
    sum, about 4 roundings per output, and the roundings of the stages add at worst linearly.  The generic butterfly sums p products
    one after another: (p - 1) u sum|terms| at worst (recursive summation), and a tone, whose terms add up coherently at its line,
    comes within a small constant of that (measured: 0.06 p u at 2 x 10223 bins, where noise shows 30 u)."""
    p, n, d = 1, nbins, 2
    while d * d <= n:
        while n % d == 0:
            p, n = d, n // d
        d += 1
    p = max(p, n)
    return u * (4 * max(1, int(np.ceil(np.log2(nbins)))) + (p if p > 5 else 0))


# ---- pcx_fft_create's choice of plan, restated ---------------------------------------------------------------------------------
def select_plan(dtype, nbins):
    """(kind, n1, n2) as pcx_fft_create (pothoscomms_amd/csrc/pcx_fft_api.hip) chooses them with no A/B switch set.  On the GPU
    Fft.plan() is the authority; this keeps the table of tests/test_fft_plans_gpu.py honest where there is none."""
    esz = {"complex_float64": 16, "complex_float32": 8, "complex_int16": 4}[dtype]
    f32, f64, i16 = esz == 8, esz == 16, esz == 4
    pow2 = nbins & (nbins - 1) == 0
    if nbins == 1:
        return "IDENTITY", 0, 0
    wg_limit = 16384 if f32 else 8192 if f64 else 4096
    r16 = pow2 and not i16 and 16 <= nbins <= wg_limit
    four_step = not i16 and pow2 and wg_limit < nbins <= wg_limit * wg_limit
    lds_limit = 160 * 1024 // (2 * esz)
    mixed_n1 = 0
    if not i16 and not pow2 and nbins > lds_limit:
        for d in range(int(np.floor(np.sqrt(float(nbins)))), 1, -1):
            if nbins % d == 0:
                if nbins // d <= lds_limit:
                    mixed_n1 = d
                break
    if not r16 and not four_step and not mixed_n1 and nbins * esz * (1 if i16 and pow2 else 2) > 160 * 1024:
        if i16:
            return "Q15_GLOBAL", 0, 0
        m = 1
        while m < 2 * nbins - 1:
            m *= 2
        return "BLUESTEIN", nbins, m
    if four_step and nbins <= ((4 << 20) if f32 else (2 << 20)):
        n1 = 256 if nbins == 65536 else 128
        if nbins // n1 > wg_limit:
            n1 = 256
        return "FOURSTEP_SHORT", n1, nbins // n1
    if four_step or mixed_n1:
        n1 = mixed_n1 or 1 << ((nbins.bit_length() - 1 + 1) // 2)
        return "FOURSTEP", n1, nbins // n1
    if f32 and nbins == 4096:
        return "R16_4096", 0, 0
    if r16:
        return "R16", 0, 0
    smooth = nbins
    for r in (2, 3, 5):
        while smooth % r == 0:
            smooth //= r
    if not pow2 and smooth == 1 and ((f32 and nbins < 8192) or (f64 and 256 <= nbins < 2048)):
        return "SMOOTH", 0, 0
    if i16:
        return ("Q15_POW2" if pow2 else "MIXED"), 0, 0
    return ("POW2" if pow2 else "MIXED"), 0, 0


# ---- metrics -------------------------------------------------------------------------------------------------------------------
def _diff(got, truth, nbins):
    g = frames(got, nbins)
    t = np.asarray(truth).reshape(-1, nbins)
    # float32 against a long-double truth: the difference taken in float64 is exact to 1e-16 of the values, 2^-29 of u
    wide = CLD if t.dtype == CLD and g.dtype != np.complex64 else np.complex128
    return g.astype(wide) - t.astype(wide), t


def rel_l2(got, truth, nbins):
    """per frame: ||got - truth||_2 / ||truth||_2"""
    d, t = _diff(got, truth, nbins)
    num = np.sqrt(np.sum(d.real ** 2 + d.imag ** 2, axis=1))
    den = np.sqrt(np.sum(t.real ** 2 + t.imag ** 2, axis=1))
    return (num / np.where(den > 0, den, 1)).astype(np.float64)


def impulse_err(got, truth, nbins):
    """max over bins of |got - truth| (every bin of an impulse's transform has modulus 1)"""
    d, _ = _diff(got, truth, nbins)
    return float(np.max(np.abs(d)))


def tone_leak(got, truth, nbins):
    """max over all bins of |got - truth| / N: the spurious level relative to the tone's line"""
    d, _ = _diff(got, truth, nbins)
    return float(np.max(np.abs(d))) / nbins
