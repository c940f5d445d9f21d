"""Thin Python handles over the C ABI (include/pcx.h) -- plumbing for tests, bench.py
and the multi-GPU stream driver.  Host arrays are numpy, device arrays are torch CUDA
(ROCm) tensors used purely as device memory; every call goes through libpcx_hip.so.

Stream layout: a complex stream of scalar type T is an array of shape (n, 2) of T
(interleaved re, im = std::complex<T>); numpy complex64/complex128 are accepted and
viewed that way.  Real streams are 1-D arrays of T.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import F64, F32, I64, I32, I16, I8, U64, U32, U16, U8  # noqa: F401  (re-exported)

NP_SCALAR = {F64: np.float64, F32: np.float32, I64: np.int64, I32: np.int32, I16: np.int16, I8: np.int8,
             U64: np.uint64, U32: np.uint32, U16: np.uint16, U8: np.uint8}   # unsigned: arithmetic, comparators, bitwise only
ARITH_OPS = {"ADD": _lib.ARITH_ADD, "SUB": _lib.ARITH_SUB, "MUL": _lib.ARITH_MUL, "DIV": _lib.ARITH_DIV}
CMP_OPS = {">": _lib.CMP_GT, "<": _lib.CMP_LT, ">=": _lib.CMP_GE, "<=": _lib.CMP_LE, "==": _lib.CMP_EQ, "!=": _lib.CMP_NE}
BIT_OPS = {"NOT": _lib.BIT_NOT, "AND": _lib.BIT_AND, "OR": _lib.BIT_OR, "XOR": _lib.BIT_XOR}
ARITHK_OPS = {"X+K": _lib.ARITHK_X_ADD_K, "X-K": _lib.ARITHK_X_SUB_K, "K-X": _lib.ARITHK_K_SUB_X, "X*K": _lib.ARITHK_X_MUL_K,
              "X/K": _lib.ARITHK_X_DIV_K, "K/X": _lib.ARITHK_K_DIV_X}
SCALAR_OF_NP = {np.dtype(v): k for k, v in NP_SCALAR.items()}

# Pothos DType names (DType::toString) -> (scalar code, is_complex)
DTYPE_NAMES = {}
for _code, _nm in ((F64, "float64"), (F32, "float32"), (I64, "int64"), (I32, "int32"), (I16, "int16"), (I8, "int8"),
                   (U64, "uint64"), (U32, "uint32"), (U16, "uint16"), (U8, "uint8")):
    DTYPE_NAMES[_nm] = (_code, False)
    DTYPE_NAMES["complex_" + _nm] = (_code, True)
DTYPE_NAMES["complex64"] = (F32, True)    # Pothos accepts numpy-style aliases
DTYPE_NAMES["complex128"] = (F64, True)
DTYPE_NAMES["float"] = (F32, False)
DTYPE_NAMES["double"] = (F64, False)


def parse_dtype(dtype):
    """'complex_float32' / np.dtype / (scalar, is_complex) -> (scalar code, is_complex)."""
    if isinstance(dtype, tuple):
        return dtype
    if isinstance(dtype, str):
        if dtype not in DTYPE_NAMES:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "unknown dtype %r" % dtype)
        return DTYPE_NAMES[dtype]
    dt = np.dtype(dtype)
    if dt == np.complex64:
        return (F32, True)
    if dt == np.complex128:
        return (F64, True)
    return (SCALAR_OF_NP[dt], False)


def as_pairs(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex64:
        return a.view(np.float32).reshape(-1, 2)
    if a.dtype == np.complex128:
        return a.view(np.float64).reshape(-1, 2)
    return a


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _dev_ptr(t):
    if not t.is_cuda:
        raise ValueError("device variant needs a CUDA/ROCm tensor")
    if not t.is_contiguous():
        raise ValueError("device buffers must be contiguous")
    return C.c_void_p(t.data_ptr())


def _any_dev_ptr(t):
    """a device tensor, or a raw device address (an int: a view at a byte offset no tensor type can express)"""
    return C.c_void_p(t) if isinstance(t, int) else _dev_ptr(t)


def _gate_ptr(t):
    """a gate word: device memory, or page-locked host memory (the device reads it in place; the host opens it with a plain store)"""
    if not t.is_cuda and t.is_pinned():
        return C.c_void_p(t.data_ptr())
    return _dev_ptr(t)


def _stream_ptr(stream=None):
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s if isinstance(s, int) else s.cuda_stream)      # a torch stream, or a raw hipStream_t


class _Handle:
    _destroy = None

    def __init__(self):
        self._h = C.c_void_p()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(_lib.load(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FirFilter(_Handle):
    """pcx_fir_*: the loop of filter/FIRFilter.cpp:278-308 behind FIRFilterFactory's type matrix."""
    _destroy = "pcx_fir_destroy"

    def __init__(self, dtype="complex_float32", taps_type="COMPLEX"):
        super().__init__()
        self.scalar, self.is_complex = parse_dtype(dtype)
        if taps_type not in ("REAL", "COMPLEX"):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "FIRFilterFactory: unsupported types")
        self.complex_taps = taps_type == "COMPLEX"
        _lib.check(_lib.load().pcx_fir_create(self.scalar, int(self.is_complex), int(self.complex_taps), C.byref(self._h)))

    def set_taps(self, taps):
        t = np.asarray(taps)
        if self.complex_taps:
            t = np.ascontiguousarray(t.astype(np.complex128)).view(np.float64)
            n = t.size // 2
        else:
            t = np.ascontiguousarray(np.real(t).astype(np.float64))
            n = t.size
        _lib.check(_lib.load().pcx_fir_set_taps(self._h, _np_ptr(t), n))

    def set_decimation(self, m):
        _lib.check(_lib.load().pcx_fir_set_decimation(self._h, m))

    def set_interpolation(self, l):
        _lib.check(_lib.load().pcx_fir_set_interpolation(self._h, l))

    def set_algo(self, algo):
        _lib.check(_lib.load().pcx_fir_set_algo(self._h, algo))

    def set_qformat(self, q):
        """pcx_fir_set_qformat: the floatToQ / fromQ reading of an integer filter -- a (frac, float_to_q, from_q) triple of the
        _lib.Q_* constants, or None for the process-wide reading"""
        _lib.check(_lib.load().pcx_fir_set_qformat(self._h, _lib.qformat_ptr(q)))

    @property
    def last_algo(self):
        return _lib.load().pcx_fir_last_algo(self._h)

    @property
    def last_plan(self):
        """pcx_fir_get_last_plan: the name (_lib.FIR_PLANS) of the plan the last call ran, "NONE" before the first"""
        v = C.c_int()
        _lib.check(_lib.load().pcx_fir_get_last_plan(self._h, C.byref(v)))
        return _lib.FIR_PLANS[v.value]

    def set_slots(self, slots):
        """pcx_fir_set_slots: the share of the device's 1024 resident workgroup slots this handle's launches take"""
        _lib.check(_lib.load().pcx_fir_set_slots(self._h, int(slots)))

    def geometry(self):
        k, r = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_fir_get_geometry(self._h, C.byref(k), C.byref(r)))
        return k.value, r.value

    @property
    def K(self):
        return self.geometry()[0]

    def process(self, inbuf, out_cap):
        """Host buffers.  Returns (out[:produced], consumed, produced)."""
        x = as_pairs(inbuf)
        n_in = x.shape[0]
        shape = (out_cap, 2) if self.is_complex else (out_cap,)
        y = np.zeros(shape, dtype=NP_SCALAR[self.scalar])
        c, p = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_fir_process(self._h, _np_ptr(x), n_in, _np_ptr(y), out_cap, C.byref(c), C.byref(p)))
        return y[:p.value], c.value, p.value

    def process_dev(self, x, y, in_elems=None, out_cap=None, stream=None):
        """Device tensors (x: in_elems elements incl. K-1 history).  Returns (consumed, produced)."""
        w = 2 if self.is_complex else 1
        if in_elems is None:
            in_elems = x.numel() // w
        if out_cap is None:
            out_cap = y.numel() // w
        c, p = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_fir_process_dev(self._h, _dev_ptr(x), in_elems, _dev_ptr(y), out_cap,
                                                   C.byref(c), C.byref(p), _stream_ptr(stream)))
        return c.value, p.value

    def process_dev_gated(self, x, y, gate, value, in_elems=None, out_cap=None, stream=None):
        """pcx_fir_process_dev_gated: one launch over a shard whose first K-1 samples (the halo) are still on their way; the blocks
        that read them wait until the 32-bit word `gate` (a device tensor) has reached `value`.  Returns (consumed, produced, gated);
        gated == False: nothing was queued (no gated kernel for this configuration)."""
        w = 2 if self.is_complex else 1
        if in_elems is None:
            in_elems = x.numel() // w
        if out_cap is None:
            out_cap = y.numel() // w
        c, p, g = C.c_size_t(), C.c_size_t(), C.c_int()
        _lib.check(_lib.load().pcx_fir_process_dev_gated(self._h, _dev_ptr(x), in_elems, _dev_ptr(y), out_cap, C.byref(c), C.byref(p),
                                                         _gate_ptr(gate), value & 0xFFFFFFFF, _stream_ptr(stream), C.byref(g)))
        return c.value, p.value, bool(g.value)


def gate_signal(gate, value, stream=None):
    """pcx_gate_signal_dev: a one-thread kernel on `stream` (default: torch's current one) that sets the gate word to `value`."""
    _lib.check(_lib.load().pcx_gate_signal_dev(_dev_ptr(gate), value & 0xFFFFFFFF, _stream_ptr(stream)))


def gate_signal_host(gate, value):
    """Open a gate that lives in page-locked HOST memory: a plain 32-bit store, no stream and no hardware queue behind it -- the way
    to signal LATE (behind the gated launch), where a stream's signal kernel could sit in the launch's own queue (include/pcx.h)."""
    if gate.is_cuda or not gate.is_pinned():
        raise ValueError("gate_signal_host needs a page-locked host tensor")
    C.c_uint32.from_address(gate.data_ptr()).value = value & 0xFFFFFFFF


class Fft(_Handle):
    """pcx_fft_*: FFTAux::transform (fft/FFTAux.h) over whole frames."""
    _destroy = "pcx_fft_destroy"

    def __init__(self, dtype, num_bins, inverse=False):
        super().__init__()
        self.scalar, cplx = parse_dtype(dtype)
        if not cplx:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "FFTFactory: unsupported type")
        self.num_bins = int(num_bins)
        _lib.check(_lib.load().pcx_fft_create(self.scalar, self.num_bins, int(bool(inverse)), C.byref(self._h)))

    def transform(self, x, nframes=None):
        xp = as_pairs(x)
        nf = xp.shape[0] // self.num_bins if nframes is None else nframes
        y = np.zeros_like(xp[:nf * self.num_bins])
        _lib.check(_lib.load().pcx_fft_transform(self._h, _np_ptr(xp), _np_ptr(y), nf))
        return y

    def transform_dev(self, x, y, nframes, stream=None):
        _lib.check(_lib.load().pcx_fft_transform_dev(self._h, _dev_ptr(x), _dev_ptr(y), nframes, _stream_ptr(stream)))

    def plan(self):
        """pcx_fft_get_plan: (name of the plan, n1, n2) -- the four-step split, or (num_bins, M) of the chirp-z plan, else 0, 0"""
        k, n1, n2 = C.c_int(), C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_fft_get_plan(self._h, C.byref(k), C.byref(n1), C.byref(n2)))
        return _lib.FFT_PLANS[k.value], n1.value, n2.value


class FreqDemod(_Handle):
    """pcx_freqdemod_*: demod/FreqDemod.cpp:44-71 with _prev carried on the device."""
    _destroy = "pcx_freqdemod_destroy"

    def __init__(self, dtype="complex_float32"):
        super().__init__()
        self.scalar, cplx = parse_dtype(dtype)
        if not cplx:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "FreqDemodFactory: unsupported types")
        _lib.check(_lib.load().pcx_freqdemod_create(self.scalar, C.byref(self._h)))

    def reset(self):
        _lib.check(_lib.load().pcx_freqdemod_reset(self._h))

    def process(self, x, out=None):
        xp = as_pairs(x)
        y = np.zeros(xp.shape[0], dtype=NP_SCALAR[self.scalar]) if out is None else out
        _lib.check(_lib.load().pcx_freqdemod_process(self._h, _np_ptr(xp), _np_ptr(y), xp.shape[0]))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_freqdemod_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


class DCRemoval(_Handle):
    """pcx_dcremoval_*: filter/DCRemoval.cpp's cascaded moving-average DC blocker, history and accumulators carried on the device.

    Integer types give the reference's bits (wrap-around included); float types are computed in exact arithmetic."""
    _destroy = "pcx_dcremoval_destroy"

    def __init__(self, dtype="complex_float32", average_size=512, cascade_size=2):
        super().__init__()
        self.dtype = dtype
        self.scalar, self.cplx = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_dcremoval_create(self.scalar, int(self.cplx), C.byref(self._h)))
        if (average_size, cascade_size) != (512, 2):
            self.set_sizes(average_size, cascade_size)

    def set_sizes(self, average_size, cascade_size):
        _lib.check(_lib.load().pcx_dcremoval_set_sizes(self._h, int(average_size), int(cascade_size)))

    def sizes(self):
        d, c = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_dcremoval_get_sizes(self._h, C.byref(d), C.byref(c)))
        return d.value, c.value

    def reset(self):
        _lib.check(_lib.load().pcx_dcremoval_reset(self._h))

    def process(self, x, out=None):
        """x: (n,) real or (n, 2) complex pairs (or a complex numpy array) of the element type"""
        x = as_pairs(x) if self.cplx else np.ascontiguousarray(x)
        if x.dtype != NP_SCALAR[self.scalar]:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "dc_removal: %s input for a %s block" % (x.dtype, self.dtype))
        if out is None:
            y = np.zeros_like(x)
        else:
            y = out
            if not (isinstance(y, np.ndarray) and y.dtype == x.dtype and y.shape == x.shape and y.flags.c_contiguous):
                raise _lib.InvalidArgument(_lib.ERR_ARG, "dc_removal: out must be a contiguous %s array of shape %s" % (x.dtype, x.shape))
        _lib.check(_lib.load().pcx_dcremoval_process(self._h, _np_ptr(x), _np_ptr(y), x.shape[0]))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_dcremoval_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


class EnvelopeDetector(_Handle):
    """pcx_envelope_*: filter/EnvelopeDetector.cpp's attack/release envelope, float32 out, bit for bit the reference's loop.

    Created as the reference constructs the block (all gains 0, lookahead 0); `attack` / `release` / `lookahead` given here are
    set through the setters.  process / process_dev take n + lookahead input elements for n outputs."""
    _destroy = "pcx_envelope_destroy"

    def __init__(self, dtype="complex_float32", attack=None, release=None, lookahead=0):
        super().__init__()
        self.dtype = dtype
        self.scalar, self.cplx = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_envelope_create(self.scalar, int(self.cplx), C.byref(self._h)))
        if attack is not None:
            self.set_attack(attack)
        if release is not None:
            self.set_release(release)
        if lookahead:
            self.set_lookahead(lookahead)

    def set_attack(self, attack):
        _lib.check(_lib.load().pcx_envelope_set_attack(self._h, float(attack)))

    def attack(self):
        v = C.c_float()
        _lib.check(_lib.load().pcx_envelope_get_attack(self._h, C.byref(v)))
        return v.value

    def set_release(self, release):
        _lib.check(_lib.load().pcx_envelope_set_release(self._h, float(release)))

    def release(self):
        v = C.c_float()
        _lib.check(_lib.load().pcx_envelope_get_release(self._h, C.byref(v)))
        return v.value

    def set_lookahead(self, lookahead):
        _lib.check(_lib.load().pcx_envelope_set_lookahead(self._h, int(lookahead)))

    def lookahead(self):
        v = C.c_size_t()
        _lib.check(_lib.load().pcx_envelope_get_lookahead(self._h, C.byref(v)))
        return v.value

    def set_warmup(self, warmup):
        """warm-up samples in front of each speculative chunk (0: derived from the gains)"""
        _lib.check(_lib.load().pcx_envelope_set_warmup(self._h, int(warmup)))

    def reset(self):
        _lib.check(_lib.load().pcx_envelope_reset(self._h))

    def state(self):
        v = C.c_float()
        _lib.check(_lib.load().pcx_envelope_get_state(self._h, C.byref(v)))
        return v.value

    def stats(self):
        """(chunks, repaired, resolved) of the last call"""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(_lib.load().pcx_envelope_get_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def process(self, x, n=None, out=None):
        """x: (m,) real or (m, 2) complex pairs (or a complex numpy array) of the element type; n outputs (default m - lookahead)
        from x[0 : n + lookahead]"""
        x = as_pairs(x) if self.cplx else np.ascontiguousarray(x)
        if x.dtype != NP_SCALAR[self.scalar] or x.ndim != (2 if self.cplx else 1):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "envelope_detector: %s%s input for a %s block" % (x.dtype, x.shape, self.dtype))
        L = self.lookahead()
        if n is None:
            n = max(0, x.shape[0] - L)
        if n + L > x.shape[0]:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "envelope_detector: %d outputs need %d input elements, %d given" % (n, n + L, x.shape[0]))
        if out is None:
            y = np.zeros(n, np.float32)
        else:
            y = out
            if not (isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (n,) and y.flags.c_contiguous):
                raise _lib.InvalidArgument(_lib.ERR_ARG, "envelope_detector: out must be a contiguous float32 array of shape (%d,)" % n)
        _lib.check(_lib.load().pcx_envelope_process(self._h, _np_ptr(x), _np_ptr(y), n))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_envelope_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


class IIRFilter(_Handle):
    """pcx_iir_*: filter/IIRFilter.cpp's recurrence in double, narrowed to the stream type.

    taps: b[0..N] followed by a[0..N]; None keeps the reference's default.  plan() says how the handle computes: (IIR_SCAN, bound)
    for a stable filter, every output within bound * max|x| of the sequential recurrence; (IIR_SERIAL, 0.0) otherwise, bit for bit."""
    _destroy = "pcx_iir_destroy"

    def __init__(self, dtype="complex_float32", taps=None):
        super().__init__()
        self.dtype = dtype
        self.scalar, self.cplx = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_iir_create(self.scalar, int(self.cplx), C.byref(self._h)))
        if taps is not None:
            self.set_taps(taps)

    def set_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
        _lib.check(_lib.load().pcx_iir_set_taps(self._h, _np_ptr(t), t.shape[0]))

    def taps(self):
        n = C.c_size_t()
        _lib.check(_lib.load().pcx_iir_get_taps(self._h, None, 0, C.byref(n)))
        t = np.zeros(n.value, np.float64)
        _lib.check(_lib.load().pcx_iir_get_taps(self._h, _np_ptr(t), t.shape[0], C.byref(n)))
        return t

    def reset(self):
        _lib.check(_lib.load().pcx_iir_reset(self._h))

    def plan(self):
        """(plan, bound): _lib.IIR_SCAN or _lib.IIR_SERIAL, and the SCAN bound per unit of max|x| (0.0 for SERIAL)"""
        p, b = C.c_int(), C.c_double()
        _lib.check(_lib.load().pcx_iir_get_plan(self._h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def process(self, x, out=None):
        """x: (n,) real or (n, 2) complex pairs (or a complex numpy array) of the element type; returns the n outputs in the same layout"""
        x = as_pairs(x) if self.cplx else np.ascontiguousarray(x)
        if x.dtype != NP_SCALAR[self.scalar] or x.ndim != (2 if self.cplx else 1) or (self.cplx and x.shape[1] != 2):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "iir_filter: %s%s input for a %s block" % (x.dtype, x.shape, self.dtype))
        if out is None:
            y = np.zeros_like(x)
        else:
            y = out
            if not (isinstance(y, np.ndarray) and y.dtype == x.dtype and y.shape == x.shape and y.flags.c_contiguous):
                raise _lib.InvalidArgument(_lib.ERR_ARG, "iir_filter: out must be a contiguous %s array of shape %s" % (x.dtype, x.shape))
        _lib.check(_lib.load().pcx_iir_process(self._h, _np_ptr(x), _np_ptr(y), x.shape[0]))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_iir_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


class Scrambler(_Handle):
    """pcx_scrambler_*: digital/Scrambler.cpp's and Descrambler.cpp's loops over the Galois LFSR of digital/lfsr.h, bit for bit
    (DESIGN.md 12).  One uint8 per bit in and out; only bit 0 of an input byte counts.

    plan() says how the handle computes: SCR_SCAN when the polynomial owns the mask's lowest bit and the seed lies below it,
    SCR_SERIAL (one thread, the reference's loop) otherwise.  state() is lfsr_t's (data, mask) after the last call."""
    _destroy = "pcx_scrambler_destroy"
    MODES = {"additive": _lib.SCR_ADDITIVE, "multiplicative": _lib.SCR_MULTIPLICATIVE}

    def __init__(self, descramble=False, mode="multiplicative", poly=0x19, seed=1):
        super().__init__()
        self.descramble = bool(descramble)
        _lib.check(_lib.load().pcx_scrambler_create(int(self.descramble), C.byref(self._h)))
        self.set_mode(mode)
        if seed != 1:
            self.set_seed(seed)
        if poly != 0x19:
            self.set_poly(poly)

    @staticmethod
    def _i64(v):
        v = int(v)
        return v - (1 << 64) if v >= (1 << 63) else v          # 0x8000000000000003 is a negative int64_t

    def set_poly(self, poly):
        _lib.check(_lib.load().pcx_scrambler_set_poly(self._h, self._i64(poly)))

    def set_seed(self, seed):
        _lib.check(_lib.load().pcx_scrambler_set_seed(self._h, self._i64(seed)))

    def set_mode(self, mode):
        if mode not in self.MODES:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "Scrambler::set_mode(): unknown mode: %s" % (mode,))
        _lib.check(_lib.load().pcx_scrambler_set_mode(self._h, self.MODES[mode]))

    def poly(self):
        v = C.c_int64()
        _lib.check(_lib.load().pcx_scrambler_get_poly(self._h, C.byref(v)))
        return v.value

    def seed(self):
        v = C.c_int64()
        _lib.check(_lib.load().pcx_scrambler_get_seed(self._h, C.byref(v)))
        return v.value

    def mode(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_scrambler_get_mode(self._h, C.byref(v)))
        return "additive" if v.value == _lib.SCR_ADDITIVE else "multiplicative"

    def plan(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_scrambler_get_plan(self._h, C.byref(v)))
        return v.value

    def state(self):
        """(data, mask) of the register as unsigned 64-bit integers, after the handle's last call"""
        d, m = C.c_int64(), C.c_int64()
        _lib.check(_lib.load().pcx_scrambler_get_state(self._h, C.byref(d), C.byref(m)))
        return d.value & (2 ** 64 - 1), m.value & (2 ** 64 - 1)

    @staticmethod
    def geometry():
        """(run, tile, group, slice): the bits a thread, a tile, a wave of the carry and a slice of the SCAN plan hold"""
        v = [C.c_size_t() for _ in range(4)]
        _lib.check(_lib.load().pcx_scrambler_get_geometry(*[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def process(self, x, out=None):
        """x: (n,) uint8; returns the n output bytes (out=x works in place)"""
        x = np.ascontiguousarray(x)
        if x.dtype != np.uint8 or x.ndim != 1:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "scrambler: %s%s input for a uint8 block" % (x.dtype, x.shape))
        if out is None:
            y = np.zeros_like(x)
        else:
            y = out
            if not (isinstance(y, np.ndarray) and y.dtype == x.dtype and y.shape == x.shape and y.flags.c_contiguous):
                raise _lib.InvalidArgument(_lib.ERR_ARG, "scrambler: out must be a contiguous uint8 array of shape %s" % (x.shape,))
        _lib.check(_lib.load().pcx_scrambler_process(self._h, _np_ptr(x), _np_ptr(y), x.shape[0]))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_scrambler_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


class PreambleCorrelator(_Handle):
    """pcx_preamble_*: digital/PreambleCorrelator.cpp's search -- the Hamming distance between the preamble and the input at every
    position, over whole bytes, and the positions where it does not exceed the threshold.  One uint8 per symbol.

    plan() says how the handle computes the distances: PRE_PLANES per bit plane of the symbols, PRE_BYTES (preambles beyond
    geometry()[2] symbols) the reference's byte loop with one position per thread."""
    _destroy = "pcx_preamble_destroy"

    def __init__(self, preamble=(1,), threshold=1):
        super().__init__()
        _lib.check(_lib.load().pcx_preamble_create(C.byref(self._h)))
        if tuple(preamble) != (1,):
            self.set_preamble(preamble)
        if threshold != 1:
            self.set_threshold(threshold)

    def set_preamble(self, preamble):
        p = np.ascontiguousarray(np.asarray(preamble, dtype=np.uint8).reshape(-1))
        _lib.check(_lib.load().pcx_preamble_set_preamble(self._h, _np_ptr(p) if p.size else None, p.size))

    def preamble(self):
        n = C.c_size_t()
        _lib.check(_lib.load().pcx_preamble_get_preamble(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        _lib.check(_lib.load().pcx_preamble_get_preamble(self._h, _np_ptr(out), out.size, C.byref(n)))
        return out

    def set_threshold(self, threshold):
        _lib.check(_lib.load().pcx_preamble_set_threshold(self._h, int(threshold)))

    def threshold(self):
        v = C.c_uint()
        _lib.check(_lib.load().pcx_preamble_get_threshold(self._h, C.byref(v)))
        return v.value

    def plan(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_preamble_get_plan(self._h, C.byref(v)))
        return v.value

    @staticmethod
    def geometry():
        """(tile, slice, max_planes_len): the positions a workgroup and a call slice hold, and the longest preamble of the PLANES plan"""
        v = [C.c_size_t() for _ in range(3)]
        _lib.check(_lib.load().pcx_preamble_get_geometry(*[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @staticmethod
    def _symbols(x):
        x = np.ascontiguousarray(x)
        if x.dtype != np.uint8 or x.ndim != 1:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "preamble correlator: %s%s input for a uint8 block" % (x.dtype, x.shape))
        return x

    def process(self, x, cap=None, out=None):
        """x: (n,) uint8 -> (label indices n + P as uint64, n_positions, n_matches).  At most `cap` indices come back (default: every
        position could match); n_matches is the full count.  out: a uint8 array that receives the n_positions forwarded bytes."""
        x = self._symbols(x)
        P = self.preamble().size
        cap = max(0, x.shape[0] - P) if cap is None else int(cap)
        idx = np.zeros(max(cap, 1), np.uint64)
        npos, nm = C.c_size_t(), C.c_size_t()
        if out is not None and not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous
                                    and out.size >= max(0, x.shape[0] - P)):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "preamble correlator: out must be a contiguous uint8 array of n - P elements")
        _lib.check(_lib.load().pcx_preamble_process(self._h, _np_ptr(x), x.shape[0], None if out is None else _np_ptr(out), _np_ptr(idx), cap,
                                                    C.byref(npos), C.byref(nm)))
        return idx[:min(nm.value, cap)].copy(), npos.value, nm.value

    def distances(self, x):
        """x: (n,) uint8 -> the n - P Hamming distances as uint32"""
        x = self._symbols(x)
        d = np.zeros(max(1, x.shape[0] - self.preamble().size), np.uint32)
        npos = C.c_size_t()
        _lib.check(_lib.load().pcx_preamble_distances(self._h, _np_ptr(x), x.shape[0], _np_ptr(d), C.byref(npos)))
        return d[:npos.value]

    def process_dev(self, x, n_in, idx, cap, counts, out=None, stream=None):
        """device tensors: x uint8, idx int64 / uint64 of at least cap elements, counts two 64-bit words that receive (n_positions,
        n_matches), out uint8 or None; nothing is allocated or synchronised"""
        c = _dev_ptr(counts).value
        _lib.check(_lib.load().pcx_preamble_process_dev(self._h, _dev_ptr(x), n_in, None if out is None else _dev_ptr(out),
                                                        _dev_ptr(idx) if cap else None, cap, C.c_void_p(c), C.c_void_p(c + 8), _stream_ptr(stream)))

    def distances_dev(self, x, n_in, dist, stream=None):
        _lib.check(_lib.load().pcx_preamble_distances_dev(self._h, _dev_ptr(x), n_in, _dev_ptr(dist), _stream_ptr(stream)))


class Threshold(_Handle):
    """pcx_threshold_*: utility/Threshold.cpp's comparison of a real stream against an activation and a deactivation level with one
    bit of carried state.  A call returns the ascending indices of the elements at which the state changed and the
    state it was entered in: transition j is an activation exactly when (state_in + j) is even.  Levels are converted to the
    element type by numpy."""
    _destroy = "pcx_threshold_destroy"

    def __init__(self, dtype="float64", activation=0, deactivation=0):
        super().__init__()
        self.dtype = dtype
        self.scalar, cplx = parse_dtype(dtype)
        if cplx:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "threshold: %s is not a real type" % (dtype,))
        _lib.check(_lib.load().pcx_threshold_create(C.byref(self._h), self.scalar))
        self.np_dtype = np.dtype(NP_SCALAR[self.scalar])
        if activation != 0 or deactivation != 0:
            self.set_levels(activation, deactivation)

    def set_levels(self, activation, deactivation):
        lv = np.array([activation, deactivation], dtype=self.np_dtype)
        _lib.check(_lib.load().pcx_threshold_set_levels(self._h, _np_ptr(lv[0:1]), _np_ptr(lv[1:2])))

    def levels(self):
        lv = np.zeros(2, self.np_dtype)
        _lib.check(_lib.load().pcx_threshold_get_levels(self._h, _np_ptr(lv[0:1]), _np_ptr(lv[1:2])))
        return lv[0], lv[1]

    def reset(self):
        _lib.check(_lib.load().pcx_threshold_reset(self._h))

    def state(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_threshold_get_state(self._h, C.byref(v)))
        return v.value

    def set_state(self, active):
        _lib.check(_lib.load().pcx_threshold_set_state(self._h, int(bool(active))))

    @staticmethod
    def geometry():
        """(tile, slice): the elements a workgroup and a call slice hold"""
        v = [C.c_size_t() for _ in range(2)]
        _lib.check(_lib.load().pcx_threshold_get_geometry(*[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _elements(self, x):
        x = np.ascontiguousarray(x)
        if x.dtype != self.np_dtype or x.ndim != 1:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "threshold: %s%s input for a %s block" % (x.dtype, x.shape, self.dtype))
        return x

    def process(self, x, cap=None, out=None):
        """x: (n,) of the element type -> (transition indices as uint64, n_transitions, state_in).  At most `cap` indices come back
        (default: every element could be a transition); n_transitions is the full count.  out: an array of the element type that
        receives the n forwarded elements (x itself: in place)."""
        x = self._elements(x)
        cap = x.shape[0] if cap is None else int(cap)
        idx = np.zeros(max(cap, 1), np.uint64)
        nt, entry = C.c_size_t(), C.c_int()
        if out is not None and not (isinstance(out, np.ndarray) and out.dtype == self.np_dtype and out.flags.c_contiguous and out.size >= x.shape[0]):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "threshold: out must be a contiguous %s array of n elements" % self.np_dtype)
        _lib.check(_lib.load().pcx_threshold_process(self._h, _np_ptr(x), x.shape[0], None if out is None else _np_ptr(out), _np_ptr(idx), cap,
                                                     C.byref(nt), C.byref(entry)))
        return idx[:min(nt.value, cap)].copy(), nt.value, entry.value

    def states(self, x):
        """x: (n,) of the element type -> the state after every element as uint8; the carried state is read and left as it is"""
        x = self._elements(x)
        s = np.zeros(max(1, x.shape[0]), np.uint8)
        _lib.check(_lib.load().pcx_threshold_states(self._h, _np_ptr(x), x.shape[0], _np_ptr(s)))
        return s[:x.shape[0]]

    def process_dev(self, x, n, idx, cap, counts, out=None, stream=None):
        """device tensors: x of the element type, idx int64 / uint64 of at least cap elements, counts three 64-bit words that receive
        (n, n_transitions, state_in), out of the element type (x itself: in place) or None; nothing is allocated or synchronised"""
        _lib.check(_lib.load().pcx_threshold_process_dev(self._h, _dev_ptr(x), n, None if out is None else _dev_ptr(out),
                                                         _dev_ptr(idx) if cap else None, cap, _dev_ptr(counts), _stream_ptr(stream)))

    def states_dev(self, x, n, states, stream=None):
        _lib.check(_lib.load().pcx_threshold_states_dev(self._h, _dev_ptr(x), n, _dev_ptr(states), _stream_ptr(stream)))


class SignalProbe(_Handle):
    """pcx_probe_*: utility/SignalProbe.cpp's value of a window of the stream -- its last element (VALUE), sqrt(sum |x|^2 / N) (RMS) or
    sum x / N (MEAN), in double precision over a fixed summation tree.  A value is a float on a real stream and a
    complex on a complex one; the *_dev forms leave pairs of doubles (re, im) in device memory."""
    _destroy = "pcx_probe_destroy"
    MODES = {"VALUE": _lib.PROBE_VALUE, "RMS": _lib.PROBE_RMS, "MEAN": _lib.PROBE_MEAN}

    def __init__(self, dtype="complex_float32", mode="VALUE", window=1024):
        super().__init__()
        self.dtype = dtype
        self.scalar, self.is_complex = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_probe_create(C.byref(self._h), self.scalar, int(self.is_complex)))
        self.np_dtype = np.dtype(NP_SCALAR[self.scalar])
        self.set_mode(mode)
        self.set_window(window)

    def set_mode(self, mode):
        if mode not in self.MODES:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "signal probe: unknown mode %r" % (mode,))
        _lib.check(_lib.load().pcx_probe_set_mode(self._h, self.MODES[mode]))
        self.mode = mode

    def set_window(self, window):
        _lib.check(_lib.load().pcx_probe_set_window(self._h, int(window)))

    @property
    def window(self):
        v = C.c_size_t()
        _lib.check(_lib.load().pcx_probe_get_window(self._h, C.byref(v)))
        return v.value

    def geometry(self):
        """(tile, slice, switch_over) in elements: the longest window of the small-window path, the slice of a longer window that a
        workgroup reduces to a partial, the shortest window of the large-window path"""
        v = [C.c_size_t() for _ in range(3)]
        _lib.check(_lib.load().pcx_probe_get_geometry(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _elements(self, x):
        x = as_pairs(x)
        if x.dtype != self.np_dtype or x.ndim != (2 if self.is_complex else 1) or (self.is_complex and x.shape[1] != 2):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "signal probe: %s%s input for a %s probe" % (x.dtype, x.shape, self.dtype))
        return x

    def _value(self, pair):
        return complex(pair[0], pair[1]) if self.is_complex else float(pair[0])

    def process(self, x):
        """one work() call on x: (value, consumed) with consumed = min(window, elements); value is None when nothing was consumed"""
        x = self._elements(x)
        v, c = np.zeros(2, np.float64), C.c_size_t()
        _lib.check(_lib.load().pcx_probe_process(self._h, _np_ptr(x), x.shape[0], _np_ptr(v), C.byref(c)))
        return (self._value(v) if c.value else None), c.value

    def windows(self, x):
        """the value of every window of x, the last one the remainder: float64 (real) or complex128 of ceil(n / window) entries"""
        x = self._elements(x)
        nw = -(-x.shape[0] // self.window)
        v = np.zeros((max(nw, 1), 2), np.float64)
        _lib.check(_lib.load().pcx_probe_windows(self._h, _np_ptr(x), x.shape[0], _np_ptr(v)))
        v = v[:nw]
        return v.copy().view(np.complex128).reshape(-1) if self.is_complex else v[:, 0].copy()

    def process_dev(self, x, n, value, stream=None):
        """device tensors (or raw device addresses): n elements at x, value two float64 that receive (re, im); returns what the call
        consumed; nothing is allocated or synchronised"""
        c = C.c_size_t()
        _lib.check(_lib.load().pcx_probe_process_dev(self._h, _any_dev_ptr(x), n, _any_dev_ptr(value), C.byref(c), _stream_ptr(stream)))
        return c.value

    def windows_dev(self, x, n, values, stream=None):
        """device tensors (or raw device addresses): values receives ceil(n / window) pairs of float64"""
        _lib.check(_lib.load().pcx_probe_windows_dev(self._h, _any_dev_ptr(x), n, _any_dev_ptr(values), _stream_ptr(stream)))


class Trigger(_Handle):
    """pcx_trigger_*: the two device parts of utility/WaveTrigger.cpp -- the least pair (y[i], y[i + 1]) of the stream converted to
    float (a complex element to its modulus) that crosses `level` with the wanted slope, and the capture of windows of W elements from
    several buffers at once.  search returns (i, y0, y1, position) or None, position being the reference's
    i + (level - y0) / (y1 - y0)."""
    _destroy = "pcx_trigger_destroy"
    SLOPES = {"POS": _lib.TRIGGER_POS, "NEG": _lib.TRIGGER_NEG, "LEVEL": _lib.TRIGGER_LEVEL}

    def __init__(self, dtype="float32", level=0.5, slope="POS"):
        super().__init__()
        self.dtype = dtype
        self.scalar, self.is_complex = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_trigger_create(C.byref(self._h), self.scalar, int(self.is_complex)))
        self.np_dtype = np.dtype(NP_SCALAR[self.scalar])
        self.elem_bytes = self.np_dtype.itemsize * (2 if self.is_complex else 1)
        self.set_level(level)
        self.set_slope(slope)

    def set_level(self, level):
        _lib.check(_lib.load().pcx_trigger_set_level(self._h, float(level)))

    @property
    def level(self):
        v = C.c_double()
        _lib.check(_lib.load().pcx_trigger_get_level(self._h, C.byref(v)))
        return v.value

    def set_slope(self, slope):
        if slope not in self.SLOPES:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "wave trigger: unknown slope setting %r" % (slope,))
        _lib.check(_lib.load().pcx_trigger_set_slope(self._h, self.SLOPES[slope]))

    @property
    def slope(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_trigger_get_slope(self._h, C.byref(v)))
        return [k for k, c in self.SLOPES.items() if c == v.value][0]

    def geometry(self):
        """the pairs a workgroup searches at a time"""
        v = C.c_size_t()
        _lib.check(_lib.load().pcx_trigger_get_geometry(self._h, C.byref(v)))
        return v.value

    def _hit(self, hit):
        if not hit.found:
            return None
        return int(hit.i), float(hit.y0), float(hit.y1), float(_lib.load().pcx_trigger_position(C.byref(hit), self.level))

    def search(self, x, start=0, n=None):
        """x: a numpy array of the element type ((n, 2) or complex for a complex type), or a raw address (host or device memory) with
        n elements behind it -> the first triggering pair at or behind `start`"""
        hit = _lib.TriggerHit()
        if isinstance(x, int):
            ptr = C.c_void_p(x)
        else:
            x = as_pairs(x)
            if x.dtype != self.np_dtype:
                raise _lib.InvalidArgument(_lib.ERR_ARG, "wave trigger: %s input for a %s trigger" % (x.dtype, self.dtype))
            ptr, n = _np_ptr(x), x.shape[0]
        _lib.check(_lib.load().pcx_trigger_search(self._h, ptr, int(n), int(start), C.byref(hit)))
        return self._hit(hit)

    def search_dev(self, x, n, start, hit, stream=None):
        """device tensors (or raw device addresses): n elements at x, hit 24 bytes that receive (uint64 i, float y0, float y1, uint64
        found); nothing is allocated or synchronised"""
        _lib.check(_lib.load().pcx_trigger_search_dev(self._h, _any_dev_ptr(x), n, int(start), _any_dev_ptr(hit), _stream_ptr(stream)))

    @staticmethod
    def _ports(ptrs):
        return (C.c_void_p * len(ptrs))(*[p if isinstance(p, int) else p.ctypes.data for p in ptrs])

    def capture(self, ins, elem_bytes, starts, W, outs=None):
        """rows [starts[e], starts[e] + W) of every buffer of `ins` (numpy uint8 arrays or raw addresses, host or device memory;
        elem_bytes[p] bytes per element) -> one (nev, W * elem_bytes[p]) uint8 matrix per buffer (or into `outs`: raw addresses)"""
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        nev = starts.shape[0]
        made = None
        if outs is None:
            made = [np.zeros((nev, W * eb), np.uint8) for eb in elem_bytes]
            outs = made
        eb = (C.c_size_t * len(ins))(*[int(e) for e in elem_bytes])
        _lib.check(_lib.load().pcx_trigger_capture(self._h, len(ins), self._ports(ins), eb, _np_ptr(starts), nev, int(W), self._ports(outs)))
        return made

    def capture_dev(self, ins, elem_bytes, starts, nev, W, outs, stream=None):
        """raw device addresses or device tensors throughout; starts: nev uint64 in device memory; nothing is allocated or synchronised"""
        addr = lambda v: [p if isinstance(p, int) else p.data_ptr() for p in v]
        eb = (C.c_size_t * len(ins))(*[int(e) for e in elem_bytes])
        _lib.check(_lib.load().pcx_trigger_capture_dev(self._h, len(ins), self._ports(addr(ins)), eb, _any_dev_ptr(starts), nev, int(W),
                                                       self._ports(addr(outs)), _stream_ptr(stream)))


class Framer(_Handle):
    """pcx_framer_*: digital/PreambleFramer.cpp (uint8) and digital/FrameInsert.cpp (complex_float32, complex_float64) -- a preamble in
    front of every start label, zero padding behind every end label, the labels of a call given as events (index, width, kind,
    length) with kind in {"other", "start", "end"} or the FRAME_* codes.  The host plans the call, one kernel writes the
    framed stream.  A call returns a FramerResult: the output, what was consumed, and per event whether it was used, where its insert
    begins and the shift of its label."""
    _destroy = "pcx_framer_destroy"
    KINDS = {"other": _lib.FRAME_OTHER, "start": _lib.FRAME_START, "end": _lib.FRAME_END}

    class Result:
        def __init__(self, out, plan, used, insert_at, shift):
            self.out, self.consumed, self.out_len, self.used_events, self.cut = out, plan.consumed, plan.out_len, plan.used_events, bool(plan.cut)
            self.n_segments, self.n_headers = plan.n_segments, plan.n_headers
            self.used, self.insert_at, self.shift = used.astype(bool), insert_at, shift

    def __init__(self, dtype="uint8", preamble=(1,), symbol_width=1, header=False, header_id=0x55, padding=0):
        super().__init__()
        self.dtype = dtype
        self.scalar, self.cplx = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_framer_create(C.byref(self._h), self.scalar, int(self.cplx)))
        self.np_dtype = np.dtype(NP_SCALAR[self.scalar])
        if tuple(np.atleast_1d(preamble).tolist()) != (1,) or symbol_width != 1 or header:
            self.set_preamble(preamble, symbol_width, header)
        if header_id != 0x55:
            self.set_header_id(header_id)
        if padding:
            self.set_padding(padding)

    def _typed(self, a, what):
        """symbols or a stream as the handle's element type: (n,) uint8 resp. (n, 2) of the scalar type"""
        if self.cplx:
            a = np.asarray(a)
            if a.ndim == 1:
                a = a.astype(np.complex64 if self.scalar == F32 else np.complex128)
            a = as_pairs(a)
            if a.dtype != self.np_dtype or a.ndim != 2 or a.shape[1] != 2:
                raise _lib.InvalidArgument(_lib.ERR_ARG, "framer: %s %s%s for a %s block" % (what, a.dtype, a.shape, self.dtype))
            return np.ascontiguousarray(a)
        a = np.ascontiguousarray(a)
        if a.dtype != np.uint8 or a.ndim != 1:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "framer: %s %s%s for a %s block" % (what, a.dtype, a.shape, self.dtype))
        return a

    def set_preamble(self, preamble, symbol_width=1, header=False):
        p = np.asarray(preamble)
        p = self._typed(p.astype(np.uint8) if not self.cplx else p, "preamble")
        _lib.check(_lib.load().pcx_framer_set_preamble(self._h, _np_ptr(p) if p.size else None, p.shape[0], int(symbol_width), int(bool(header))))

    def preamble(self):
        """(symbols, symbol_width, header)"""
        n, w, hd = C.c_size_t(), C.c_size_t(), C.c_int()
        _lib.check(_lib.load().pcx_framer_get_preamble(self._h, None, 0, C.byref(n), C.byref(w), C.byref(hd)))
        out = np.zeros((n.value, 2) if self.cplx else n.value, self.np_dtype)
        _lib.check(_lib.load().pcx_framer_get_preamble(self._h, _np_ptr(out), n.value, C.byref(n), C.byref(w), C.byref(hd)))
        return out, w.value, bool(hd.value)

    def set_header_id(self, header_id):
        _lib.check(_lib.load().pcx_framer_set_header_id(self._h, int(header_id) & 0xFF))

    def header_id(self):
        v = C.c_ubyte()
        _lib.check(_lib.load().pcx_framer_get_header_id(self._h, C.byref(v)))
        return v.value

    def set_padding(self, padding):
        _lib.check(_lib.load().pcx_framer_set_padding(self._h, int(padding)))

    def padding(self):
        v = C.c_size_t()
        _lib.check(_lib.load().pcx_framer_get_padding(self._h, C.byref(v)))
        return v.value

    @staticmethod
    def geometry():
        """(tile_bytes, lds_segments): the output bytes a workgroup writes and the longest slice of the segment table it keeps on chip"""
        v = [C.c_size_t() for _ in range(2)]
        _lib.check(_lib.load().pcx_framer_get_geometry(*[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @staticmethod
    def header_bits(header_id, length):
        """the 58 header bits as an int: bit i belongs to the i-th header symbol"""
        v = C.c_uint64()
        _lib.check(_lib.load().pcx_frame_header_bits(int(header_id), int(length), C.byref(v)))
        return v.value

    @classmethod
    def events(cls, events):
        """[(index, width, kind, length)] -> a ctypes array of pcx_frame_event (at least one entry long) and the count; such a pair
        passes through (a caller that reuses its events builds them once)"""
        if isinstance(events, tuple) and len(events) == 2 and isinstance(events[0], C.Array):
            return events
        arr = (_lib.FrameEvent * max(1, len(events)))()
        for e, (index, width, kind, length) in zip(arr, events):
            e.index, e.width, e.kind, e.length = int(index), int(width), cls.KINDS.get(kind, kind), int(length) & 0xFFFF
        return arr, len(events)

    @staticmethod
    def _per_event(n):
        return np.zeros(max(1, n), np.uint8), np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64)

    def plan(self, n_in, out_cap, events, tables=True):
        """host only: (Result without output, segments [(dst, kind, src)] with the sentinel, header words); tables=False leaves the last
        two out (None) and plans once"""
        ev, n = self.events(events)
        plan = _lib.FramePlan()
        used, at, shift = self._per_event(n)
        L = _lib.load()
        if not tables:
            _lib.check(L.pcx_framer_plan(self._h, n_in, out_cap, ev, n, C.byref(plan), _np_ptr(used), _np_ptr(at), _np_ptr(shift), None, 0, None, 0))
            return self.Result(None, plan, used[:n], at[:n], shift[:n]), None, None
        # an event leaves at most three segments (its head, the sync word, the header or the padding) and one header word; the tail and
        # the sentinel are two more
        segs = (_lib.FrameSegment * (3 * n + 2))()
        hdr = np.zeros(max(1, n), np.uint64)
        _lib.check(L.pcx_framer_plan(self._h, n_in, out_cap, ev, n, C.byref(plan), _np_ptr(used), _np_ptr(at), _np_ptr(shift), segs, 3 * n + 2,
                                     _np_ptr(hdr), n))
        return (self.Result(None, plan, used[:n], at[:n], shift[:n]), [(g.dst, g.kind, g.src) for g in segs[:plan.n_segments]],
                [int(v) for v in hdr[:plan.n_headers]])

    def process(self, x, events=(), out_cap=None, out=None):
        """x: the stream as a numpy array; out_cap: room of the output in elements (default: what the whole input needs); out: an array
        of the element type with room for out_cap elements"""
        x = self._typed(x, "input")
        ev, n = self.events(events)
        if out_cap is None:
            pre, w, hd = self.preamble()
            out_cap = x.shape[0] + n * (pre.shape[0] * w + (_lib.FRAME_HEADER_BITS if hd else 0) + self.padding()) if out is None else out.shape[0]
        shape = (max(1, out_cap), 2) if self.cplx else (max(1, out_cap),)
        if out is None:
            out = np.zeros(shape, self.np_dtype)
        elif not (isinstance(out, np.ndarray) and out.dtype == self.np_dtype and out.flags.c_contiguous and out.shape[0] >= out_cap and out.shape[1:] == shape[1:]):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "framer: out must be a contiguous %s array with room for out_cap elements" % self.np_dtype)
        plan = _lib.FramePlan()
        used, at, shift = self._per_event(n)
        _lib.check(_lib.load().pcx_framer_process(self._h, _np_ptr(x) if x.shape[0] else None, x.shape[0], ev, n, _np_ptr(out), out_cap, C.byref(plan),
                                                  _np_ptr(used), _np_ptr(at), _np_ptr(shift)))
        return self.Result(out[:plan.out_len], plan, used[:n], at[:n], shift[:n])

    def process_dev(self, x, n_in, events, out, out_cap, stream=None):
        """device tensors x and out (torch, used as memory: out_cap elements of room from out's first byte); the events stay on the host.
        Enqueues on the stream and returns the Result without output; nothing is synchronised"""
        ev, n = self.events(events)
        plan = _lib.FramePlan()
        used, at, shift = self._per_event(n)
        _lib.check(_lib.load().pcx_framer_process_dev(self._h, _dev_ptr(x) if n_in else None, n_in, ev, n, _dev_ptr(out), out_cap, C.byref(plan),
                                                      _np_ptr(used), _np_ptr(at), _np_ptr(shift), _stream_ptr(stream)))
        return self.Result(None, plan, used[:n], at[:n], shift[:n])


class FrameSync(_Handle):
    """pcx_fsync_*: digital/FrameSync.cpp (complex_float32, complex_float64) -- the search for /comms/frame_insert's sync word, the
    header behind it and the payload behind that.  One call is one work() of the reference; the handle carries its state
    and activate() resets it.  A call returns a Result: the output, what was consumed and produced, the port's reserve, the labels
    [(kind, index, width, value)] with kind in {"phase_offset", "frame_start", "frame_end"} (value: the phase, else the length) and
    the state after the call."""
    _destroy = "pcx_fsync_destroy"
    MODES = ("RAW", "PHASE", "TIMING", "DEBUG")
    LABEL_KINDS = ("phase_offset", "frame_start", "frame_end")

    class Result:
        def __init__(self, out, r):
            self.out, self.consumed, self.produced, self.reserve = out, r.consumed, r.produced, r.reserve
            self.labels = [(FrameSync.LABEL_KINDS[l.kind], l.index, l.width, l.value if l.kind == 0 else l.length) for l in r.labels[:r.n_labels]]
            self.remaining, self.phase, self.phase_inc = r.remaining, r.phase, r.phase_inc
            self.scale, self.delta_fc, self.phase_off = r.scale, r.delta_fc, r.phase_off
            self.max_peak, self.count_since_max = r.max_peak, r.count_since_max

    def __init__(self, dtype="complex_float32", output_mode="RAW", preamble=(1,), header_id=0x55, symbol_width=20, data_width=4,
                 input_threshold=0.01, frame_start_id="frameStart", frame_end_id="", phase_offset_id=""):
        super().__init__()
        self.dtype = dtype
        self.scalar, self.cplx = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_fsync_create(C.byref(self._h), self.scalar, int(self.cplx)))
        self.np_dtype = np.dtype(NP_SCALAR[self.scalar])
        self.set_output_mode(output_mode)
        self.set_symbol_width(symbol_width)
        self.set_data_width(data_width)
        self.set_preamble(preamble)
        self.set_header_id(header_id)
        self.set_input_threshold(input_threshold)
        self.set_label_ids(frame_start_id, frame_end_id, phase_offset_id)

    def _typed(self, a, what):
        a = np.asarray(a)
        if a.ndim == 1:
            a = a.astype(np.complex64 if self.scalar == F32 else np.complex128)
        a = as_pairs(a)
        if a.dtype != self.np_dtype or a.ndim != 2 or a.shape[1] != 2:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "frame sync: %s %s%s for a %s block" % (what, a.dtype, a.shape, self.dtype))
        return np.ascontiguousarray(a)

    def set_output_mode(self, mode):
        if mode not in self.MODES:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "FrameSync::setOutputMode(%s): unknown output mode" % (mode,))
        _lib.check(_lib.load().pcx_fsync_set_output_mode(self._h, self.MODES.index(mode)))

    def output_mode(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_fsync_get_output_mode(self._h, C.byref(v)))
        return self.MODES[v.value]

    def set_preamble(self, preamble):
        p = self._typed(np.asarray(preamble), "preamble")
        _lib.check(_lib.load().pcx_fsync_set_preamble(self._h, _np_ptr(p) if p.size else None, p.shape[0]))

    def preamble(self):
        n = C.c_size_t()
        _lib.check(_lib.load().pcx_fsync_get_preamble(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 2), self.np_dtype)
        _lib.check(_lib.load().pcx_fsync_get_preamble(self._h, _np_ptr(out), n.value, C.byref(n)))
        return out

    def set_header_id(self, header_id):
        _lib.check(_lib.load().pcx_fsync_set_header_id(self._h, int(header_id) & 0xFF))

    def header_id(self):
        v = C.c_ubyte()
        _lib.check(_lib.load().pcx_fsync_get_header_id(self._h, C.byref(v)))
        return v.value

    def set_symbol_width(self, width):
        _lib.check(_lib.load().pcx_fsync_set_symbol_width(self._h, int(width)))

    def symbol_width(self):
        v = C.c_size_t()
        _lib.check(_lib.load().pcx_fsync_get_symbol_width(self._h, C.byref(v)))
        return v.value

    def set_data_width(self, width):
        _lib.check(_lib.load().pcx_fsync_set_data_width(self._h, int(width)))

    def data_width(self):
        v = C.c_size_t()
        _lib.check(_lib.load().pcx_fsync_get_data_width(self._h, C.byref(v)))
        return v.value

    def set_input_threshold(self, threshold):
        _lib.check(_lib.load().pcx_fsync_set_input_threshold(self._h, float(threshold)))

    def input_threshold(self):
        v = C.c_double()
        _lib.check(_lib.load().pcx_fsync_get_input_threshold(self._h, C.byref(v)))
        return v.value

    def set_verbose(self, enable):
        _lib.check(_lib.load().pcx_fsync_set_verbose(self._h, int(bool(enable))))

    def set_label_ids(self, frame_start_id=None, frame_end_id=None, phase_offset_id=None):
        """None leaves an id as it is; an empty id switches the label off"""
        for kind, v in ((1, frame_start_id), (2, frame_end_id), (0, phase_offset_id)):
            if v is not None:
                _lib.check(_lib.load().pcx_fsync_set_label_id(self._h, kind, str(v).encode()))

    def label_ids(self):
        """(frame_start_id, frame_end_id, phase_offset_id)"""
        out = []
        for kind in (1, 2, 0):
            n = C.c_size_t()
            _lib.check(_lib.load().pcx_fsync_get_label_id(self._h, kind, None, 0, C.byref(n)))
            buf = C.create_string_buffer(n.value + 1)
            _lib.check(_lib.load().pcx_fsync_get_label_id(self._h, kind, buf, n.value + 1, C.byref(n)))
            out.append(buf.value.decode())
        return tuple(out)

    def geometry(self):
        """(sync_width, frame_width, corr_mag, corr_dur, tile, first_piece): the derived settings, the offsets a workgroup of the search
        owns and the offsets of a search call's first piece"""
        v = [C.c_size_t() for _ in range(6)]
        _lib.check(_lib.load().pcx_fsync_get_geometry(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def activate(self):
        _lib.check(_lib.load().pcx_fsync_activate(self._h))

    def process(self, x, out_cap=None, out=None):
        """x: the call's input as a numpy array; out_cap: room of the output in elements (default: as many as the input)"""
        x = self._typed(x, "input")
        if out_cap is None:
            out_cap = x.shape[0] if out is None else out.shape[0]
        if out is None:
            out = np.zeros((max(1, out_cap), 2), self.np_dtype)
        elif not (isinstance(out, np.ndarray) and out.dtype == self.np_dtype and out.flags.c_contiguous and out.shape[0] >= out_cap and out.shape[1:] == (2,)):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "frame sync: out must be a contiguous %s array with room for out_cap elements" % self.np_dtype)
        r = _lib.FsyncResult()
        _lib.check(_lib.load().pcx_fsync_process(self._h, _np_ptr(x) if x.shape[0] else None, x.shape[0], _np_ptr(out), out_cap, C.byref(r)))
        return self.Result(out[:r.produced], r)

    def process_dev(self, x, n_in, out, out_cap, stream=None):
        """device memory x and out (torch tensors used as memory, or raw addresses); returns the Result without output.  A search call
        waits for the stream, a payload call only enqueues"""
        r = _lib.FsyncResult()
        _lib.check(_lib.load().pcx_fsync_process_dev(self._h, _any_dev_ptr(x) if n_in else None, n_in, _any_dev_ptr(out) if out_cap else None, out_cap,
                                                     C.byref(r), _stream_ptr(stream)))
        return self.Result(None, r)


class _SymbolMap(_Handle):
    """what pcx_mapper_* and pcx_slicer_* share: a map in the stream type's own element layout"""
    _family = None

    def __init__(self, dtype="complex_float32", map=None):
        super().__init__()
        self.scalar, self.is_complex = parse_dtype(dtype)
        _lib.check(getattr(_lib.load(), self._family + "_create")(self.scalar, int(self.is_complex), C.byref(self._h)))
        if map is not None:
            self.set_map(map)

    def _typed(self, m):
        """a map as an array of the stream type: (n,) for a real stream, (n, 2) for a complex one.  An array that already has the
        stream's scalar type is taken as it is (so an int64 map is exact); anything else goes through complex128 / float64."""
        t = NP_SCALAR[self.scalar]
        a = np.asarray(m)
        if self.is_complex:
            if a.dtype == t and a.ndim == 2 and a.shape[1] == 2:
                return np.ascontiguousarray(a)
            c = a.astype(np.complex128).reshape(-1)
            return np.ascontiguousarray(np.stack([c.real, c.imag], axis=1).astype(t))
        if a.dtype == t:
            return np.ascontiguousarray(a.reshape(-1))
        return np.ascontiguousarray(np.real(a).astype(np.float64).astype(t).reshape(-1))

    def set_map(self, m):
        a = self._typed(m)
        _lib.check(getattr(_lib.load(), self._family + "_set_map")(self._h, _np_ptr(a) if a.size else None, a.shape[0]))

    def map(self):
        """the map as last set, in the stream type: (n,) or (n, 2)"""
        n = C.c_size_t()
        get = getattr(_lib.load(), self._family + "_get_map")
        _lib.check(get(self._h, None, 0, C.byref(n)))
        a = np.zeros([n.value] + ([2] if self.is_complex else []), dtype=NP_SCALAR[self.scalar])
        _lib.check(get(self._h, _np_ptr(a), n.value, C.byref(n)))
        return a

    def _stream(self, x, what):
        x = np.ascontiguousarray(as_pairs(x))
        want = 2 if self.is_complex else 1
        if x.dtype != NP_SCALAR[self.scalar] or x.ndim != want or (self.is_complex and x.shape[1] != 2):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "%s: %s%s for a %s%s stream" % (what, x.dtype, x.shape, "complex " if self.is_complex else "",
                                                                                       np.dtype(NP_SCALAR[self.scalar]).name))
        return x


class SymbolMapper(_SymbolMap):
    """pcx_mapper_*: digital/SymbolMapper.cpp's loop, out[i] = map[in[i] & mask].  uint8 in, the stream type out."""
    _destroy = "pcx_mapper_destroy"
    _family = "pcx_mapper"

    def process(self, x):
        x = np.ascontiguousarray(x)
        if x.dtype != np.uint8 or x.ndim != 1:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "symbol mapper: %s%s input for a uint8 block" % (x.dtype, x.shape))
        y = np.zeros([x.shape[0]] + ([2] if self.is_complex else []), dtype=NP_SCALAR[self.scalar])
        _lib.check(_lib.load().pcx_mapper_process(self._h, _np_ptr(x), _np_ptr(y), x.shape[0]))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_mapper_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


class SymbolSlicer(_SymbolMap):
    """pcx_slicer_*: digital/SymbolSlicer.cpp's loop -- the first map entry with the strictly smallest float distance, as a byte
    (DESIGN.md 14).  The stream type in, uint8 out."""
    _destroy = "pcx_slicer_destroy"
    _family = "pcx_slicer"

    def geometry(self):
        """(lane, group, max_onchip_map, slice): samples a lane and a workgroup hold, the longest map held on chip, elements per call slice"""
        v = [C.c_size_t() for _ in range(4)]
        _lib.check(_lib.load().pcx_slicer_get_geometry(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def process(self, x):
        x = self._stream(x, "symbol slicer")
        y = np.zeros(x.shape[0], dtype=np.uint8)
        _lib.check(_lib.load().pcx_slicer_process(self._h, _np_ptr(x), _np_ptr(y), x.shape[0]))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_slicer_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


class DifferentialCoder(_Handle):
    """pcx_diffcode_*: digital/DifferentialEncoder.cpp's and DifferentialDecoder.cpp's loops, byte for byte.  One uint8
    per symbol in and out; the carried byte survives calls and set_symbols.

    plan() says how the handle computes: DIFF_SCAN when the encoder's step is a modular prefix sum for this symbols (checked over all
    65536 byte pairs), DIFF_SERIAL (one thread, the reference's loop) otherwise; the decoder always reports DIFF_SCAN."""
    _destroy = "pcx_diffcode_destroy"

    def __init__(self, decode=False, symbols=2):
        super().__init__()
        self.decode = bool(decode)
        _lib.check(_lib.load().pcx_diffcode_create(int(self.decode), C.byref(self._h)))
        if symbols != 2:
            self.set_symbols(symbols)

    def set_symbols(self, symbols):
        symbols = int(symbols)
        if not 0 <= symbols < 1 << 32:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "symbols is a uint32_t: %d" % symbols)
        _lib.check(_lib.load().pcx_diffcode_set_symbols(self._h, symbols))

    def symbols(self):
        v = C.c_uint32()
        _lib.check(_lib.load().pcx_diffcode_get_symbols(self._h, C.byref(v)))
        return v.value

    def plan(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_diffcode_get_plan(self._h, C.byref(v)))
        return v.value

    def state(self):
        """the carried byte after the handle's last call"""
        v = C.c_ubyte()
        _lib.check(_lib.load().pcx_diffcode_get_state(self._h, C.byref(v)))
        return v.value

    def reset(self):
        _lib.check(_lib.load().pcx_diffcode_reset(self._h))

    @staticmethod
    def geometry():
        """(tile, slice): the bytes a workgroup and a call slice hold"""
        t, s = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_diffcode_get_geometry(C.byref(t), C.byref(s)))
        return t.value, s.value

    def process(self, x, out=None):
        """x: (n,) uint8; returns the n output bytes (out=x works in place)"""
        x = np.ascontiguousarray(x)
        if x.dtype != np.uint8 or x.ndim != 1:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "differential coder: %s%s input for a uint8 block" % (x.dtype, x.shape))
        if out is None:
            y = np.zeros_like(x)
        else:
            y = out
            if not (isinstance(y, np.ndarray) and y.dtype == x.dtype and y.shape == x.shape and y.flags.c_contiguous):
                raise _lib.InvalidArgument(_lib.ERR_ARG, "differential coder: out must be a contiguous uint8 array of shape %s" % (x.shape,))
        _lib.check(_lib.load().pcx_diffcode_process(self._h, _np_ptr(x), _np_ptr(y), x.shape[0]))
        return y

    def process_dev(self, x, y, n, stream=None):
        _lib.check(_lib.load().pcx_diffcode_process_dev(self._h, _dev_ptr(x), _dev_ptr(y), n, _stream_ptr(stream)))


REPACK_KINDS = {"bits_to_symbols": _lib.REPACK_BITS_TO_SYMBOLS, "symbols_to_bits": _lib.REPACK_SYMBOLS_TO_BITS,
                "bytes_to_symbols": _lib.REPACK_BYTES_TO_SYMBOLS, "symbols_to_bytes": _lib.REPACK_SYMBOLS_TO_BYTES}


class SymbolRepacker(_Handle):
    """pcx_repack_*: the four conversions of digital/SymbolHelpers.hpp between bits (one per byte), symbols of `modulus` bits (one per
    byte) and payload bytes, byte for byte.  uint8 in and out, nothing carried between calls.

    A fresh handle holds the reference's constructor values: modulus 1, "MSBit" for the two bit kinds, "LSBit" for the two byte
    kinds.  A call takes a whole number of group()[0] input elements and gives group()[1] outputs for each."""
    _destroy = "pcx_repack_destroy"

    def __init__(self, kind, modulus=None, bit_order=None):
        super().__init__()
        if kind not in REPACK_KINDS:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "repack: unknown kind %r (%s)" % (kind, ", ".join(sorted(REPACK_KINDS))))
        self.kind = kind
        _lib.check(_lib.load().pcx_repack_create(REPACK_KINDS[kind], C.byref(self._h)))
        if modulus is not None:
            self.set_modulus(modulus)
        if bit_order is not None:
            self.set_bit_order(bit_order)

    def set_modulus(self, modulus):
        modulus = int(modulus)
        _lib.check(_lib.load().pcx_repack_set_modulus(self._h, modulus if 0 <= modulus < 1 << 32 else 0))

    def modulus(self):
        v = C.c_uint()
        _lib.check(_lib.load().pcx_repack_get_modulus(self._h, C.byref(v)))
        return v.value

    def set_bit_order(self, order):
        if order not in ("LSBit", "MSBit"):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "Order must be LSBit or MSBit")
        _lib.check(_lib.load().pcx_repack_set_bit_order(self._h, int(order == "MSBit")))

    def bit_order(self):
        v = C.c_int()
        _lib.check(_lib.load().pcx_repack_get_bit_order(self._h, C.byref(v)))
        return "MSBit" if v.value else "LSBit"

    def group(self):
        """(in, out): the indivisible unit the reference reserves, in input and output elements"""
        a, b = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_repack_get_group(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def geometry(self):
        """(tile, slice): the input elements a workgroup and a call slice hold at the handle's setting"""
        t, s = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_repack_get_geometry(self._h, C.byref(t), C.byref(s)))
        return t.value, s.value

    def out_elems(self, n):
        gin, gout = self.group()
        return n // gin * gout

    def process(self, x):
        """x: (n,) uint8, a whole number of groups; returns the n / group()[0] * group()[1] output bytes"""
        x = np.ascontiguousarray(x)
        if x.dtype != np.uint8 or x.ndim != 1:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "repack: %s%s input for a uint8 block" % (x.dtype, x.shape))
        y = np.zeros(self.out_elems(x.shape[0]), np.uint8)
        _lib.check(_lib.load().pcx_repack_process(self._h, _np_ptr(x), _np_ptr(y), x.shape[0]))
        return y

    def process_dev(self, x, out, n, stream=None):
        """x, out: CUDA/ROCm uint8 tensors or raw device addresses; n input elements"""
        ptr = lambda t: C.c_void_p(t) if isinstance(t, int) else _dev_ptr(t)      # noqa: E731
        _lib.check(_lib.load().pcx_repack_process_dev(self._h, ptr(x), ptr(out), n, _stream_ptr(stream)))
        return out


WAVES = {"CONST": _lib.WAVE_CONST, "SINE": _lib.WAVE_SINE, "RAMP": _lib.WAVE_RAMP, "SQUARE": _lib.WAVE_SQUARE}
NOISE_WAVES = {"UNIFORM": _lib.NOISE_UNIFORM, "NORMAL": _lib.NOISE_NORMAL, "LAPLACE": _lib.NOISE_LAPLACE, "POISSON": _lib.NOISE_POISSON}


def waveform_table(dtype, wave, rate=1.0, freq=0.0, res=0.0, ampl=1.0, offset=0.0):
    """pcx_waveform_table: (table, step) of the waveform source at these settings, built on the host as WaveformSource.cpp:178-259
    builds it.  ampl and offset are complex.  The table is (entries, 2) for a complex type, (entries,) for a real one."""
    scalar, cplx = parse_dtype(dtype)
    if wave not in WAVES:
        raise _lib.InvalidArgument(_lib.ERR_ARG, "unknown waveform setting")
    ampl, offset = complex(ampl), complex(offset)
    args = (scalar, int(cplx), WAVES[wave], float(rate), float(freq), float(res), ampl.real, ampl.imag, offset.real, offset.imag)
    entries, step = C.c_size_t(), C.c_uint64()
    _lib.check(_lib.load().pcx_waveform_table(*args, None, 0, C.byref(entries), C.byref(step)))
    table = np.zeros((entries.value, 2) if cplx else (entries.value,), NP_SCALAR[scalar])
    _lib.check(_lib.load().pcx_waveform_table(*args, _np_ptr(table), entries.value, C.byref(entries), C.byref(step)))
    return table, step.value


class NoiseGenerator(_Handle):
    """pcx_noise_*: the std::mt19937 of the noise source and its four distributions as NoiseSource.cpp:188-250 calls them (host only).
    seed None: from std::random_device, as the reference's constructor does."""
    _destroy = "pcx_noise_destroy"

    def __init__(self, seed=None):
        super().__init__()
        _lib.check(_lib.load().pcx_noise_create(int(seed is not None), int(seed or 0) & 0xFFFFFFFF, C.byref(self._h)))

    def table(self, dtype, wave, mean=0.0, b=1.0, ampl=1.0, offset=0.0):
        """the next 4096-entry table of the generator (every call draws on)"""
        scalar, cplx = parse_dtype(dtype)
        if wave not in NOISE_WAVES:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "unknown waveform setting")
        ampl, offset = complex(ampl), complex(offset)
        table = np.zeros((_lib.NOISE_ENTRIES, 2) if cplx else (_lib.NOISE_ENTRIES,), NP_SCALAR[scalar])
        _lib.check(_lib.load().pcx_noise_table(self._h, scalar, int(cplx), NOISE_WAVES[wave], float(mean), float(b), ampl.real, ampl.imag,
                                               offset.real, offset.imag, _np_ptr(table)))
        return table

    def next_offset(self):
        """the draw in front of every work(): uniform over 0 ... 4095"""
        v = C.c_size_t()
        _lib.check(_lib.load().pcx_noise_next_offset(self._h, C.byref(v)))
        return v.value


class TableSource(_Handle):
    """pcx_source_*: the cyclic walk of a table of the stream type from a carried 64-bit index, out[i] = table[(index + i * step) &
    (entries - 1)].  The index is host state and advances when a call is made."""
    _destroy = "pcx_source_destroy"

    def __init__(self, dtype):
        super().__init__()
        self.scalar, self.cplx = parse_dtype(dtype)
        _lib.check(_lib.load().pcx_source_create(self.scalar, int(self.cplx), C.byref(self._h)))

    def set_table(self, table, step, entries=None):
        """table: (entries, 2) resp. (entries,) of the stream type, or any contiguous array of that many bytes with `entries` given"""
        t = as_pairs(table)
        _lib.check(_lib.load().pcx_source_set_table(self._h, _np_ptr(t), t.shape[0] if entries is None else int(entries), int(step) & ((1 << 64) - 1)))

    def index(self):
        v = C.c_uint64()
        _lib.check(_lib.load().pcx_source_get_index(self._h, C.byref(v)))
        return v.value

    def set_index(self, index):
        _lib.check(_lib.load().pcx_source_set_index(self._h, int(index) & ((1 << 64) - 1)))

    def geometry(self):
        """(tile, period, staged): elements per workgroup pass, elements after which the stream repeats, whether the period sits in LDS"""
        t, p, s = C.c_size_t(), C.c_size_t(), C.c_int()
        _lib.check(_lib.load().pcx_source_get_geometry(self._h, C.byref(t), C.byref(p), C.byref(s)))
        return t.value, p.value, bool(s.value)

    def generate(self, n, out=None, stream=None):
        """the next n elements: into a fresh numpy array, into `out` (numpy: on return; a CUDA/ROCm tensor or a raw device address:
        enqueued on `stream`)"""
        n = int(n)
        if out is None:
            out = np.zeros((n, 2) if self.cplx else (n,), NP_SCALAR[self.scalar])
        if isinstance(out, np.ndarray):
            if not out.flags.c_contiguous or out.dtype != NP_SCALAR[self.scalar] or out.size < n * (2 if self.cplx else 1):
                raise _lib.InvalidArgument(_lib.ERR_ARG, "source: %s%s output for %d elements" % (out.dtype, out.shape, n))
            _lib.check(_lib.load().pcx_source_generate(self._h, _np_ptr(out), n))
            return out
        ptr = C.c_void_p(out) if isinstance(out, int) else _dev_ptr(out)
        _lib.check(_lib.load().pcx_source_generate_dev(self._h, ptr, n, _stream_ptr(stream)))
        return out


class WaveformSource(TableSource):
    """/comms/waveform_source without the block around it: the settings of WaveformSource.cpp, the table built on the host from them
    at once (there is no activation here) and walked on the device.  The index survives every setter."""

    def __init__(self, dtype="complex_float32", wave="CONST", rate=1.0, freq=0.0, res=0.0, ampl=1.0, offset=0.0):
        super().__init__(dtype)
        self._dtype = (self.scalar, self.cplx)
        self.settings = dict(wave=wave, rate=rate, freq=freq, res=res, ampl=ampl, offset=offset)
        self.update()

    def update(self, **settings):
        """change any of wave, rate, freq, res, ampl, offset and rebuild the table"""
        unknown = set(settings) - set(self.settings)
        if unknown:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "waveform source: unknown setting %s" % ", ".join(sorted(unknown)))
        self.settings.update(settings)
        self.table, self.step = waveform_table(self._dtype, **self.settings)
        self.set_table(self.table, self.step)


class NoiseSource(TableSource):
    """/comms/noise_source without the block around it: a NoiseGenerator, its table at the settings, and the draw that moves the
    index in front of every generate()."""

    def __init__(self, dtype="complex_float32", wave="NORMAL", mean=0.0, b=1.0, ampl=1.0, offset=0.0, seed=None):
        super().__init__(dtype)
        self._dtype = (self.scalar, self.cplx)
        self.gen = NoiseGenerator(seed)
        self.settings = dict(wave=wave, mean=mean, b=b, ampl=ampl, offset=offset)
        self.update()

    def update(self, **settings):
        unknown = set(settings) - set(self.settings)
        if unknown:
            raise _lib.InvalidArgument(_lib.ERR_ARG, "noise source: unknown setting %s" % ", ".join(sorted(unknown)))
        self.settings.update(settings)
        self.table = self.gen.table(self._dtype, **self.settings)
        self.set_table(self.table, 1)

    def generate(self, n, out=None, stream=None):
        self.set_index(self.index() + self.gen.next_offset())
        return super().generate(n, out, stream)

    def close(self):
        self.gen.close()
        super().close()


class FmChain(_Handle):
    """pcx_fmchain_*: Rotate -> FIR -> FreqDemod in one kernel (complex_float32 -> float32)."""
    _destroy = "pcx_fmchain_destroy"

    def __init__(self):
        super().__init__()
        _lib.check(_lib.load().pcx_fmchain_create(C.byref(self._h)))

    def set_phase(self, phase):
        _lib.check(_lib.load().pcx_fmchain_set_phase(self._h, float(phase)))

    def set_taps(self, taps, complex_taps=None):
        t = np.asarray(taps)
        if complex_taps is None:
            complex_taps = np.iscomplexobj(t)
        if complex_taps:
            t = np.ascontiguousarray(t.astype(np.complex128)).view(np.float64)
            n = t.size // 2
        else:
            t = np.ascontiguousarray(np.real(t).astype(np.float64))
            n = t.size
        _lib.check(_lib.load().pcx_fmchain_set_taps(self._h, _np_ptr(t), n, int(bool(complex_taps))))

    def reset(self):
        _lib.check(_lib.load().pcx_fmchain_reset(self._h))

    def set_algo(self, algo):
        _lib.check(_lib.load().pcx_fmchain_set_algo(self._h, algo))

    @property
    def last_algo(self):
        return _lib.load().pcx_fmchain_last_algo(self._h)

    def set_slots(self, slots):
        _lib.check(_lib.load().pcx_fmchain_set_slots(self._h, int(slots)))

    def process(self, x, out_cap):
        xp = as_pairs(x)
        y = np.zeros(out_cap, dtype=np.float32)
        c, p = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_fmchain_process(self._h, _np_ptr(xp), xp.shape[0], _np_ptr(y), out_cap, C.byref(c), C.byref(p)))
        return y[:p.value], c.value, p.value

    def process_dev(self, x, y, in_elems, out_cap, stream=None):
        c, p = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().pcx_fmchain_process_dev(self._h, _dev_ptr(x), in_elems, _dev_ptr(y), out_cap,
                                                       C.byref(c), C.byref(p), _stream_ptr(stream)))
        return c.value, p.value

    def process_dev_gated(self, x, y, gate, value, in_elems, out_cap, stream=None):
        """pcx_fmchain_process_dev_gated (see FirFilter.process_dev_gated; the halo is K samples).  Returns (consumed, produced, gated)."""
        c, p, g = C.c_size_t(), C.c_size_t(), C.c_int()
        _lib.check(_lib.load().pcx_fmchain_process_dev_gated(self._h, _dev_ptr(x), in_elems, _dev_ptr(y), out_cap, C.byref(c), C.byref(p),
                                                             _gate_ptr(gate), value & 0xFFFFFFFF, _stream_ptr(stream), C.byref(g)))
        return c.value, p.value, bool(g.value)


# ---- stateless maps ------------------------------------------------------------------
def _map(host_fn, dev_fn, scalar_args, x, out_shape_fn, n, out=None, stream=None):
    L = _lib.load()
    if _is_torch(x):
        _lib.check(getattr(L, dev_fn)(*scalar_args, _dev_ptr(x), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    y = np.zeros(out_shape_fn(x), dtype=x.dtype) if out is None else out
    _lib.check(getattr(L, host_fn)(*scalar_args, _np_ptr(x), _np_ptr(y), n))
    return y


_libm = None


def _polar(phase):
    """std::polar(1.0, phase) as an optimised C++ build evaluates it (Rotate.cpp:74): GCC merges the cos and
    sin of one argument into a single glibc sincos() call, whose sine differs from sin() in the last bit for
    some arguments (e.g. 2.747554270528532) -- and so do numpy's own vector routines.  The block layer
    (comms_blocks.cpp) gets this for free; the Python wrapper asks libm for the same call."""
    global _libm
    if _libm is None:
        try:
            _libm = C.CDLL("libm.so.6")
            _libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            _libm.sincos.restype = None
        except (OSError, AttributeError):
            _libm = False
    if not _libm:
        return math.cos(phase), math.sin(phase)
    s, c = C.c_double(), C.c_double()
    _libm.sincos(phase, C.byref(s), C.byref(c))
    return c.value, s.value


def set_qformat(q=None):
    """pcx_set_qformat: the process-wide floatToQ / fromQ reading (a (frac, float_to_q, from_q) triple; None: the built-in default)"""
    _lib.check(_lib.load().pcx_set_qformat(_lib.qformat_ptr(q)))


def get_qformat():
    q = _lib.QFormat()
    _lib.check(_lib.load().pcx_get_qformat(C.byref(q)))
    return (q.frac, q.float_to_q, q.from_q)


def rotate(x, phase, scalar=None, out=None, n=None, stream=None, qformat=None):
    """arrayRotate (math/Rotate.cpp:15-23).  phase=None: block whose setPhase was never called.  qformat: pcx_rotate_q's reading."""
    pr, pi = (0.0, 0.0) if phase is None else _polar(float(phase))
    if not _is_torch(x):
        x = as_pairs(x)
        scalar, n = SCALAR_OF_NP[x.dtype], x.shape[0]
    if qformat is not None:
        return _map("pcx_rotate_q", "pcx_rotate_q_dev", (scalar, pr, pi, _lib.qformat_ptr(qformat)), x, lambda a: a.shape, n, out, stream)
    return _map("pcx_rotate", "pcx_rotate_dev", (scalar, pr, pi), x, lambda a: a.shape, n, out, stream)


def scale(x, factor, is_complex, scalar=None, out=None, n=None, stream=None, qformat=None):
    if not _is_torch(x):
        x = as_pairs(x)
        scalar, n = SCALAR_OF_NP[x.dtype], x.shape[0]
    if qformat is not None:
        return _map("pcx_scale_q", "pcx_scale_q_dev", (scalar, int(is_complex), float(factor), _lib.qformat_ptr(qformat)), x, lambda a: a.shape, n, out, stream)
    return _map("pcx_scale", "pcx_scale_dev", (scalar, int(is_complex), float(factor)), x, lambda a: a.shape, n, out, stream)


def abs_(x, is_complex, scalar=None, out=None, n=None, stream=None):
    if not _is_torch(x):
        x = as_pairs(x)
        scalar, n = SCALAR_OF_NP[x.dtype], x.shape[0]
    return _map("pcx_abs", "pcx_abs_dev", (scalar, int(is_complex)), x, lambda a: (a.shape[0],), n, out, stream)


def conj(x, scalar=None, out=None, n=None, stream=None):
    if not _is_torch(x):
        x = as_pairs(x)
        scalar, n = SCALAR_OF_NP[x.dtype], x.shape[0]
    return _map("pcx_conj", "pcx_conj_dev", (scalar,), x, lambda a: a.shape, n, out, stream)


def angle(x, scalar=None, out=None, n=None, stream=None):
    """getAngle per element (math/Angle.cpp): complex in, real out."""
    if not _is_torch(x):
        x = as_pairs(x)
        scalar, n = SCALAR_OF_NP[x.dtype], x.shape[0]
    return _map("pcx_angle", "pcx_angle_dev", (scalar,), x, lambda a: (a.shape[0],), n, out, stream)


def arith(op, a, b, is_complex, scalar=None, out=None, n=None, stream=None):
    """out[i] = a[i] OP b[i], OP in "ADD"/"SUB"/"MUL"/"DIV" (math/Arithmetic.cpp:70-110, factory :279-297).
    torch operands: device buffers (out may be a or b); numpy: host path."""
    L = _lib.load()
    if op not in ARITH_OPS:
        raise _lib.InvalidArgument(_lib.ERR_ARG, "arithmeticFactory: unsupported args (operation %r)" % (op,))
    if _is_torch(a):
        _lib.check(L.pcx_arith_dev(scalar, int(is_complex), ARITH_OPS[op], _dev_ptr(a), _dev_ptr(b), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    a, b = as_pairs(a), as_pairs(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("operands must match")
    y = np.zeros_like(a) if out is None else out
    _lib.check(L.pcx_arith(SCALAR_OF_NP[a.dtype], int(is_complex), ARITH_OPS[op], _np_ptr(a), _np_ptr(b), _np_ptr(y), a.shape[0]))
    return y


def _op_code(table, op, what):
    if op not in table:
        raise _lib.InvalidArgument(_lib.ERR_ARG, "%s: unknown operation %r" % (what, op))
    return table[op]


def _const_elem(k, scalar, is_complex=False):
    """the constant as ONE element of the stream's type: a number, a complex number (complex streams), or an array that holds the element"""
    dt = NP_SCALAR[scalar]
    if isinstance(k, np.ndarray) and k.dtype == dt and k.size == (2 if is_complex else 1):
        return np.ascontiguousarray(k).reshape(-1)
    if is_complex:
        k = complex(k) if np.isscalar(k) else complex(k[0], k[1])
        return np.array([k.real, k.imag]).astype(dt)
    return np.array([k]).astype(dt)


def compare(op, a, b, scalar=None, out=None, n=None, stream=None):
    """out[i] = (a[i] OP b[i]) ? 1 : 0 as uint8, OP in ">" "<" ">=" "<=" "==" "!=" (math/Comparator.cpp).  torch operands: device buffers of
    n scalars of type `scalar`; numpy: host path."""
    L, code = _lib.load(), _op_code(CMP_OPS, op, "comparator")
    if _is_torch(a):
        _lib.check(L.pcx_compare_dev(scalar, code, _dev_ptr(a), _dev_ptr(b), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("operands must match")
    y = np.zeros(a.size, dtype=np.uint8) if out is None else out
    _lib.check(L.pcx_compare(SCALAR_OF_NP[a.dtype], code, _np_ptr(a), _np_ptr(b), _np_ptr(y), a.size))
    return y


def compare_const(op, x, k, scalar=None, out=None, n=None, stream=None):
    """out[i] = (x[i] OP k) ? 1 : 0 as uint8 (math/ConstComparator.cpp); k is converted to the stream's type"""
    L, code = _lib.load(), _op_code(CMP_OPS, op, "const comparator")
    if _is_torch(x):
        _lib.check(L.pcx_compare_const_dev(scalar, code, _dev_ptr(x), _np_ptr(_const_elem(k, scalar)), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    x = np.ascontiguousarray(x)
    scalar = SCALAR_OF_NP[x.dtype]
    y = np.zeros(x.size, dtype=np.uint8) if out is None else out
    _lib.check(L.pcx_compare_const(scalar, code, _np_ptr(x), _np_ptr(_const_elem(k, scalar)), _np_ptr(y), x.size))
    return y


def bitwise(op, ins, scalar=None, out=None, n=None, stream=None):
    """"NOT" of one input, or "AND" / "OR" / "XOR" folded over two inputs or more in one pass (digital/Bitwise.cpp); `out` may be one of them"""
    L, code = _lib.load(), _op_code(BIT_OPS, op, "bitwise")
    ins = [ins] if _is_torch(ins) or isinstance(ins, np.ndarray) else list(ins)
    if ins and _is_torch(ins[0]):
        ptrs = (C.c_void_p * len(ins))(*[_dev_ptr(t) for t in ins])
        _lib.check(L.pcx_bitwise_dev(scalar, code, ptrs, len(ins), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    ins = [np.ascontiguousarray(a) for a in ins]
    if any(a.shape != ins[0].shape or a.dtype != ins[0].dtype for a in ins):
        raise ValueError("operands must match")
    if not ins:
        _lib.check(L.pcx_bitwise(U8 if scalar is None else scalar, code, None, 0, None, 0))
    y = np.zeros_like(ins[0]) if out is None else out
    ptrs = (C.c_void_p * len(ins))(*[a.ctypes.data for a in ins])
    _lib.check(L.pcx_bitwise(SCALAR_OF_NP[ins[0].dtype], code, ptrs, len(ins), _np_ptr(y), ins[0].size))
    return y


def bitwise_const(op, x, k, scalar=None, out=None, n=None, stream=None):
    """out[i] = x[i] OP k, OP in "AND" / "OR" / "XOR" (digital/Bitwise.cpp)"""
    L, code = _lib.load(), _op_code(BIT_OPS, op, "const bitwise")
    if _is_torch(x):
        _lib.check(L.pcx_bitwise_const_dev(scalar, code, _dev_ptr(x), _np_ptr(_const_elem(k, scalar)), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    x = np.ascontiguousarray(x)
    scalar = SCALAR_OF_NP[x.dtype]
    y = np.zeros_like(x) if out is None else out
    _lib.check(L.pcx_bitwise_const(scalar, code, _np_ptr(x), _np_ptr(_const_elem(k, scalar)), _np_ptr(y), x.size))
    return y


def bitshift(left, x, shift, scalar=None, out=None, n=None, stream=None):
    """out[i] = x[i] << shift (left) or x[i] >> shift, as C++ on the promoted value (digital/Bitwise.cpp); shift below the bit width"""
    L = _lib.load()
    if shift < 0:
        raise _lib.InvalidArgument(_lib.ERR_ARG, "bitshift: a negative shift")
    if _is_torch(x):
        _lib.check(L.pcx_bitshift_dev(scalar, int(bool(left)), _dev_ptr(x), int(shift), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    x = np.ascontiguousarray(x)
    y = np.zeros_like(x) if out is None else out
    _lib.check(L.pcx_bitshift(SCALAR_OF_NP[x.dtype], int(bool(left)), _np_ptr(x), int(shift), _np_ptr(y), x.size))
    return y


def math_fn(name, x, param=None, out=None, stream=None):
    """out[i] = f(x[i]) for one function of pcx_math_fn, by name ("EXP" ... "SIGMOID", the 24 operations of /comms/trigonometric, and
    with `param` "EXPN" (base), "LOGN" (base), "POW" (exponent), "NTH_ROOT" (root)); float32 and float64.  A numpy array goes the host
    path, a device tensor stays on the device (`out` may be x itself; a new tensor by default)."""
    L = _lib.load()
    code = _op_code(_lib.MATH_FN, str(name).upper(), "math function")
    if _is_torch(x):
        import torch
        scalar = {torch.float64: F64, torch.float32: F32}.get(x.dtype, I8)      # (any other type: refused by the call, as for numpy)
        out = torch.empty_like(x) if out is None else out
        ptrs, n, tail = (_dev_ptr(x), _dev_ptr(out)), x.numel(), (_stream_ptr(stream),)
        host_fn, par_fn = L.pcx_mathfn_dev, L.pcx_mathfn_param_dev
    else:
        x = np.ascontiguousarray(x)
        scalar = SCALAR_OF_NP.get(x.dtype, I8)
        out = np.zeros_like(x) if out is None else out
        ptrs, n, tail = (_np_ptr(x), _np_ptr(out)), x.size, ()
        host_fn, par_fn = L.pcx_mathfn, L.pcx_mathfn_param
    if param is None:
        _lib.check(host_fn(scalar, code, *ptrs, n, *tail))
    else:
        k = np.array([param]).astype(NP_SCALAR[scalar] if scalar in (F64, F32) else np.float64)
        _lib.check(par_fn(scalar, code, _np_ptr(k), *ptrs, n, *tail))
    return out


def _float_operands(*xs):
    """(scalar, element count) of operands that must agree in kind, type and size; a type the calls refuse maps to I8"""
    x = xs[0]
    if _is_torch(x):
        import torch
        if any(not _is_torch(a) or a.dtype != x.dtype or a.numel() != x.numel() for a in xs):
            raise _lib.InvalidArgument(_lib.ERR_ARG, "operands must be device tensors of one type and size")
        return {torch.float64: F64, torch.float32: F32}.get(x.dtype, I8), x.numel()
    if any(_is_torch(a) or a.dtype != x.dtype or a.size != x.size for a in xs):
        raise _lib.InvalidArgument(_lib.ERR_ARG, "operands must be arrays of one type and size")
    return SCALAR_OF_NP.get(x.dtype, I8), x.size


def special_fn(name, x, out=None, stream=None):
    """out[i] = f(x[i]) for one function of pcx_spec_fn, by name: "GAMMA", "LNGAMMA", "ERF", "ERFC"; float32 and float64.  A numpy
    array goes the host path, a device tensor stays on the device (`out` may be x itself; a new tensor by default)."""
    L = _lib.load()
    code = _op_code(_lib.SPEC_FN, str(name).upper(), "special function")
    if _is_torch(x):
        import torch
        out = torch.empty_like(x) if out is None else out
        scalar, n = _float_operands(x, out)
        _lib.check(L.pcx_specfn_dev(scalar, code, _dev_ptr(x), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    x = np.ascontiguousarray(x)
    out = np.zeros_like(x) if out is None else out
    scalar, n = _float_operands(x, out)
    _lib.check(L.pcx_specfn(scalar, code, _np_ptr(x), _np_ptr(out), n))
    return out


def beta(a, b, out=None, stream=None):
    """out[i] = exp(lgamma(a[i]) + lgamma(b[i]) - lgamma(a[i] + b[i])), the beta function as std::beta computes it (its magnitude where
    an argument is negative); float32 and float64, a and b of one type and size.  `out` may be a or b itself."""
    L = _lib.load()
    if _is_torch(a):
        import torch
        out = torch.empty_like(a) if out is None else out
        scalar, n = _float_operands(a, b, out)
        _lib.check(L.pcx_beta_dev(scalar, _dev_ptr(a), _dev_ptr(b), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.zeros_like(a) if out is None else out
    scalar, n = _float_operands(a, b, out)
    _lib.check(L.pcx_beta(scalar, _np_ptr(a), _np_ptr(b), _np_ptr(out), n))
    return out


def modf(x, out_int=None, out_frac=None, stream=None):
    """(int, frac) with frac[i] = std::modf(x[i], &int[i]): the integral and the fractional part, both with the sign of x[i]; float32
    and float64.  Either output may be x itself; the two outputs share nothing."""
    L = _lib.load()
    if _is_torch(x):
        import torch
        out_int = torch.empty_like(x) if out_int is None else out_int
        out_frac = torch.empty_like(x) if out_frac is None else out_frac
        scalar, n = _float_operands(x, out_int, out_frac)
        _lib.check(L.pcx_modf_dev(scalar, _dev_ptr(x), _dev_ptr(out_int), _dev_ptr(out_frac), n, _stream_ptr(stream)))
        return out_int, out_frac
    x = np.ascontiguousarray(x)
    out_int = np.zeros_like(x) if out_int is None else out_int
    out_frac = np.zeros_like(x) if out_frac is None else out_frac
    scalar, n = _float_operands(x, out_int, out_frac)
    _lib.check(L.pcx_modf(scalar, _np_ptr(x), _np_ptr(out_int), _np_ptr(out_frac), n))
    return out_int, out_frac


def byteswap(x, width=None, out=None, n=None, stream=None):
    """every scalar of `width` = 2, 4 or 8 bytes reversed (digital/ByteOrder.hpp); n counts scalars, a complex element is two"""
    L = _lib.load()
    if _is_torch(x):
        _lib.check(L.pcx_byteswap_dev(width, _dev_ptr(x), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    x = as_pairs(x)
    y = np.zeros_like(x) if out is None else out
    _lib.check(L.pcx_byteswap(x.dtype.itemsize if width is None else width, _np_ptr(x), _np_ptr(y), x.size))
    return y


def arith_const(op, x, k, is_complex, scalar=None, out=None, n=None, stream=None):
    """out[i] = x[i] OP k or k OP x[i], op in "X+K" "X-K" "K-X" "X*K" "X/K" "K/X" (math/ConstArithmetic.cpp), the operators of arith()"""
    L, code = _lib.load(), _op_code(ARITHK_OPS, op, "const arithmetic")
    if _is_torch(x):
        _lib.check(L.pcx_arith_const_dev(scalar, int(is_complex), code, _dev_ptr(x), _np_ptr(_const_elem(k, scalar, is_complex)), _dev_ptr(out), n,
                                         _stream_ptr(stream)))
        return out
    x = as_pairs(x)
    scalar = SCALAR_OF_NP[x.dtype]
    y = np.zeros_like(x) if out is None else out
    _lib.check(L.pcx_arith_const(scalar, int(is_complex), code, _np_ptr(x), _np_ptr(_const_elem(k, scalar, is_complex)), _np_ptr(y), x.shape[0]))
    return y


def split_complex(x, scalar=None, re=None, im=None, n=None, stream=None):
    """arraySplitComplex (utility/SplitComplex.cpp:10-18): (n, 2) interleaved -> two planes."""
    L = _lib.load()
    if _is_torch(x):
        _lib.check(L.pcx_split_complex_dev(scalar, _dev_ptr(x), _dev_ptr(re), _dev_ptr(im), n, _stream_ptr(stream)))
        return re, im
    x = as_pairs(x)
    re = np.zeros(x.shape[0], dtype=x.dtype) if re is None else re
    im = np.zeros(x.shape[0], dtype=x.dtype) if im is None else im
    _lib.check(L.pcx_split_complex(SCALAR_OF_NP[x.dtype], _np_ptr(x), _np_ptr(re), _np_ptr(im), x.shape[0]))
    return re, im


def combine_complex(re, im, scalar=None, out=None, n=None, stream=None):
    """arrayCombineComplex (utility/CombineComplex.cpp:10-17)."""
    L = _lib.load()
    if _is_torch(re):
        _lib.check(L.pcx_combine_complex_dev(scalar, _dev_ptr(re), _dev_ptr(im), _dev_ptr(out), n, _stream_ptr(stream)))
        return out
    re, im = np.ascontiguousarray(re), np.ascontiguousarray(im)
    y = np.zeros((re.shape[0], 2), dtype=re.dtype) if out is None else out
    _lib.check(L.pcx_combine_complex(SCALAR_OF_NP[re.dtype], _np_ptr(re), _np_ptr(im), _np_ptr(y), re.shape[0]))
    return y


def fill_uniform_f32_dev(t, seed, offset=0, stream=None):
    """Fill a float32 CUDA tensor with the deterministic synthetic stream (uniform [-1,1))."""
    _lib.check(_lib.load().pcx_fill_uniform_f32_dev(_dev_ptr(t), t.numel(), seed, offset, _stream_ptr(stream)))
    return t


def clock_probe(out, spin_us, stream):
    """pcx_clock_probe_dev: one wave on `stream` (a raw stream pointer or torch stream) spins for spin_us and writes the shader clock in
    MHz to the float32 CUDA tensor `out`."""
    _lib.check(_lib.load().pcx_clock_probe_dev(_dev_ptr(out), int(spin_us), _stream_ptr(stream)))


class NodeStream(_Handle):
    """pcx_shard_*: ONE complex_float32 stream over several devices from ONE process -- per-device FIR handles and
    streams, the tap-length halo exchanged natively by RCCL send/recv (or peer copies), include/pcx.h."""
    _destroy = "pcx_shard_destroy"
    RCCL, PEER_COPY = 0, 1

    def __init__(self, devices, transport=0):
        super().__init__()
        devs = (C.c_int * len(devices))(*devices)
        _lib.check(_lib.load().pcx_shard_create(len(devices), devs, transport, C.byref(self._h)))
        self.nshards = len(devices)

    def set_taps(self, taps, complex_taps=True):
        t = np.asarray(taps)
        if complex_taps:
            t = np.ascontiguousarray(t.astype(np.complex128)).view(np.float64)
            n = t.size // 2
        else:
            t = np.ascontiguousarray(np.real(t).astype(np.float64))
            n = t.size
        _lib.check(_lib.load().pcx_shard_set_taps(self._h, t.ctypes.data_as(C.POINTER(C.c_double)), n, int(complex_taps)))
        self.K = n

    def set_algo(self, algo):
        _lib.check(_lib.load().pcx_shard_set_algo(self._h, algo))

    def set_gated(self, enable):
        """pcx_shard_set_gated: False = two launches per shard and pass (body, halo event, head) instead of one gated launch"""
        _lib.check(_lib.load().pcx_shard_set_gated(self._h, int(bool(enable))))

    def set_submit_threads(self, enable):
        """pcx_shard_set_submit_threads: one thread per device queues that device's share of a pass"""
        _lib.check(_lib.load().pcx_shard_set_submit_threads(self._h, int(bool(enable))))

    def set_chain(self, enable, phase=0.0):
        """pcx_shard_set_chain: the shards run Rotate(phase) -> FIR -> FreqDemod (float32 outputs, halo of K samples)."""
        _lib.check(_lib.load().pcx_shard_set_chain(self._h, int(bool(enable)), float(phase)))
        self.chain = bool(enable)

    def configure(self, shard_elems):
        _lib.check(_lib.load().pcx_shard_configure(self._h, shard_elems))
        self.C = shard_elems

    def info(self):
        """pcx_shard_info -> (nshards, K, shard_elems, transport) as the handle holds them"""
        n, K, Ce, t = C.c_int(), C.c_size_t(), C.c_size_t(), C.c_int()
        _lib.check(_lib.load().pcx_shard_info(self._h, C.byref(n), C.byref(K), C.byref(Ce), C.byref(t)))
        return n.value, K.value, Ce.value, t.value

    def buffers(self, g):
        """(in_dev, out_dev, stream, device) of shard g as integers."""
        i, o, s, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        _lib.check(_lib.load().pcx_shard_buffers(self._h, g, C.byref(i), C.byref(o), C.byref(s), C.byref(d)))
        return i.value, o.value, s.value, d.value

    def scatter(self, x):
        xp = as_pairs(x)
        _lib.check(_lib.load().pcx_shard_scatter(self._h, _np_ptr(xp), xp.shape[0]))

    def step(self):
        _lib.check(_lib.load().pcx_shard_step(self._h))

    def post_exchange(self):
        """pcx_shard_post_exchange: the halos of what the shard buffers hold now start travelling (double-buffered streaming over two NodeStreams)"""
        _lib.check(_lib.load().pcx_shard_post_exchange(self._h))

    def compute(self):
        """pcx_shard_compute: the pass whose exchange post_exchange() queued"""
        _lib.check(_lib.load().pcx_shard_compute(self._h))

    def sync(self):
        _lib.check(_lib.load().pcx_shard_sync(self._h))

    def gather(self, out=None):
        shape = (self.nshards * self.C,) if getattr(self, "chain", False) else (self.nshards * self.C, 2)
        y = np.empty(shape, np.float32) if out is None else out
        _lib.check(_lib.load().pcx_shard_gather(self._h, _np_ptr(y), y.shape[0]))
        return y
