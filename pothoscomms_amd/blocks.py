"""Python face of the host-side block layer (libpcx_blocks.so, include/pcx_blocks.h).

`make(path, dtype, ...)` is BlockRegistry::make for the MI355X-backed /comms blocks; the
returned Block exposes the registered calls by name (`call("setTaps", taps)`), `activate()`
and `work(inbuf, out_elems, labels)` -- one scheduler work() on host buffers, returning what
the block consumed / produced / reserved and the labels it posted.  Used by the tests to show
the blocks behave like the reference blocks; inside Pothos the same C++ blocks load as a
plugin module and this wrapper is not involved.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .device import NP_SCALAR, as_pairs, parse_dtype

_HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS_LIB_PATH = os.path.join(_HERE, "libpcx_blocks.so")
NONE, SIZE, DOUBLE, STRING = 0, 1, 2, 3
_SIZE_MAX = C.c_size_t(-1).value


class PcxbArg(C.Structure):
    """pcxb_arg: one factory argument behind the dtype (pcxb_make_args)"""
    _fields_ = [("kind", C.c_int), ("uval", C.c_uint64), ("ival", C.c_int64), ("dval", C.c_double), ("dim", C.c_double), ("sval", C.c_char_p)]


INT64, COMPLEX = 4, 5


def _factory_arg(a):
    """a string, a count (int), or a constant of the stream's type given as a float, a complex or a numpy integer"""
    c = PcxbArg()
    if isinstance(a, str):
        c.kind, c.sval = STRING, a.encode()
    elif isinstance(a, (complex, np.complexfloating)):
        c.kind, c.dval, c.dim = COMPLEX, float(a.real), float(a.imag)
    elif isinstance(a, (float, np.floating)):
        c.kind, c.dval = DOUBLE, float(a)
    elif isinstance(a, np.integer) or (isinstance(a, int) and a < 0):
        v = int(a)
        c.kind, c.ival = INT64, v - (1 << 64) if v >= (1 << 63) else v
    else:
        c.kind, c.uval = SIZE, int(a)
    return c


class PcxbLabel(C.Structure):
    _fields_ = [("id", C.c_char * 32), ("index", C.c_uint64), ("width", C.c_uint64), ("kind", C.c_int),
                ("uval", C.c_uint64), ("dval", C.c_double), ("sval", C.c_char * 32)]


_blib = None
# the module libraries: "comms" is libpcx_blocks.so (comms_blocks.cpp, fir_designer.cpp), "filter" libpcx_filter_blocks.so
# (filter_blocks.cpp: /comms/dc_removal), "envelope" libpcx_envelope_blocks.so (envelope_blocks.cpp: /comms/envelope_detector), "iir"
# libpcx_iir_blocks.so (iir_blocks.cpp: /comms/iir_filter), "digital" libpcx_digital_blocks.so (digital_blocks.cpp: /comms/scrambler,
# /comms/descrambler), "correlator" libpcx_correlator_blocks.so (correlator_blocks.cpp: /comms/preamble_correlator), "symbol"
# libpcx_symbol_blocks.so (symbol_blocks.cpp: /comms/symbol_mapper, /comms/symbol_slicer, /comms/differential_encoder,
# /comms/differential_decoder), "repack" libpcx_repack_blocks.so (repack_blocks.cpp: /comms/bits_to_symbols, /comms/symbols_to_bits,
# /comms/bytes_to_symbols, /comms/symbols_to_bytes), "waveform" libpcx_waveform_blocks.so (waveform_blocks.cpp: /comms/waveform_source,
# /comms/noise_source), "utility" libpcx_utility_blocks.so (utility_blocks.cpp: /comms/threshold), "framer" libpcx_framer_blocks.so
# (framer_blocks.cpp: /comms/preamble_framer, /comms/frame_insert), "logic" libpcx_logic_blocks.so (logic_blocks.cpp: /comms/comparator,
# /comms/const_comparator, /comms/const_arithmetic, /comms/bitwise_unary, /comms/bitwise_binary, /comms/const_bitwise_binary,
# /comms/bitshift, /comms/byte_order), "math" libpcx_math_blocks.so (math_blocks.cpp: /comms/exp, exp2, exp10, expm1, expN, log, log2, log10,
# log1p, logN, pow, sqrt, cbrt, nth_root, rsqrt, sinc, sigmoid, trigonometric), "special" libpcx_special_blocks.so (special_blocks.cpp:
# /comms/gamma, lngamma, erf, erfc, beta, modf), "probe" libpcx_probe_blocks.so (probe_blocks.cpp: /comms/signal_probe, a block without
# an output port), "framesync" libpcx_framesync_blocks.so (framesync_blocks.cpp: /comms/frame_sync) -- one registry each, as Pothos loads one module library per source directory
MODULES = {"comms": BLOCKS_LIB_PATH, "filter": os.path.join(_HERE, "libpcx_filter_blocks.so"),
           "envelope": os.path.join(_HERE, "libpcx_envelope_blocks.so"), "iir": os.path.join(_HERE, "libpcx_iir_blocks.so"),
           "digital": os.path.join(_HERE, "libpcx_digital_blocks.so"), "correlator": os.path.join(_HERE, "libpcx_correlator_blocks.so"),
           "symbol": os.path.join(_HERE, "libpcx_symbol_blocks.so"), "repack": os.path.join(_HERE, "libpcx_repack_blocks.so"),
           "waveform": os.path.join(_HERE, "libpcx_waveform_blocks.so"), "utility": os.path.join(_HERE, "libpcx_utility_blocks.so"),
           "framer": os.path.join(_HERE, "libpcx_framer_blocks.so"), "logic": os.path.join(_HERE, "libpcx_logic_blocks.so"),
           "math": os.path.join(_HERE, "libpcx_math_blocks.so"), "special": os.path.join(_HERE, "libpcx_special_blocks.so"),
           "probe": os.path.join(_HERE, "libpcx_probe_blocks.so"), "framesync": os.path.join(_HERE, "libpcx_framesync_blocks.so"),
           # "trigger" libpcx_trigger_blocks.so (trigger_blocks.cpp: /comms/wave_trigger, input ports without a type, messages on its output)
           "trigger": os.path.join(_HERE, "libpcx_trigger_blocks.so")}
MSG_OTHER, MSG_PACKET, MSG_LABEL = 0, 1, 2
HAS_INDEX, HAS_POSITION, HAS_LEVEL = 1, 2, 4
_mlibs = {}


def load(module="comms"):
    global _blib
    if module == "comms" and _blib is not None:
        return _blib
    if module in _mlibs:
        return _mlibs[module]
    _lib.load()    # one HIP runtime per process, libpcx_hip.so first
    if module not in MODULES:
        raise ValueError("no block module %r (%s)" % (module, ", ".join(sorted(MODULES))))
    path = MODULES[module]
    if module == "comms":
        path = os.environ.get("PCX_BLOCKS_LIBRARY") or path     # the override selects the sanitizer build (make asan)
    if not os.path.exists(path):
        raise ImportError("%s is missing: build with make -C pothoscomms_amd/csrc" % path)
    L = C.CDLL(path)
    vp, sz, i, cp = C.c_void_p, C.c_size_t, C.c_int, C.c_char_p
    L.pcxb_last_error.restype = cp
    L.pcxb_registry_has.argtypes = [cp]
    L.pcxb_registry_count.restype = sz
    L.pcxb_registry_path.restype = cp
    L.pcxb_registry_path.argtypes = [sz]
    L.pcxb_registry_arity.restype = C.c_long
    L.pcxb_registry_arity.argtypes = [cp]
    L.pcxb_call_count.argtypes = [vp, C.POINTER(sz)]
    L.pcxb_call_name.argtypes = [vp, sz, cp, sz]
    L.pcxb_call_arity.restype = C.c_long
    L.pcxb_call_arity.argtypes = [vp, cp]
    L.pcxb_make.argtypes = [cp, cp, sz, cp, sz, i, C.POINTER(vp)]
    L.pcxb_make_args.argtypes = [cp, cp, sz, C.POINTER(PcxbArg), sz, C.POINTER(vp)]
    L.pcxb_destroy.argtypes = [vp]
    L.pcxb_call_double.argtypes = [vp, cp, C.c_double]
    L.pcxb_call_size.argtypes = [vp, cp, sz]
    L.pcxb_call_bool.argtypes = [vp, cp, i]
    L.pcxb_call_int64.argtypes = [vp, cp, C.c_int64]
    L.pcxb_get_int64.argtypes = [vp, cp, C.POINTER(C.c_int64)]
    L.pcxb_call_bytes.argtypes = [vp, cp, vp, sz]
    L.pcxb_get_bytes.argtypes = [vp, cp, vp, sz, C.POINTER(sz)]
    L.pcxb_call_string.argtypes = [vp, cp, cp]
    L.pcxb_call_taps.argtypes = [vp, cp, vp, sz, i]
    L.pcxb_get_double.argtypes = [vp, cp, C.POINTER(C.c_double)]
    L.pcxb_call_complex.argtypes = [vp, cp, C.c_double, C.c_double]
    L.pcxb_get_complex.argtypes = [vp, cp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pcxb_get_size.argtypes = [vp, cp, C.POINTER(sz)]
    L.pcxb_call_void.argtypes = [vp, cp]
    L.pcxb_input_reserve.argtypes = [vp, C.POINTER(sz)]
    L.pcxb_get_bool.argtypes = [vp, cp, C.POINTER(i)]
    L.pcxb_get_string.argtypes = [vp, cp, cp, sz]
    L.pcxb_get_taps.argtypes = [vp, cp, vp, sz, C.POINTER(sz), i]
    L.pcxb_activate.argtypes = [vp]
    L.pcxb_deactivate.argtypes = [vp]
    L.pcxb_connect_signal.argtypes = [vp, cp, vp, cp]
    L.pcxb_port_dtype.argtypes = [vp, i, cp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.pcxb_buffer_manager.argtypes = [vp, i, cp, sz, C.POINTER(sz)]
    L.pcxb_initial_reserve.argtypes = [vp, C.POINTER(sz)]
    L.pcxb_acquire_buffer.argtypes = [vp, i, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
    L.pcxb_link_buffer.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
    L.pcxb_work_loop.argtypes = [vp, vp, sz, vp, sz, sz, C.POINTER(C.c_double), C.POINTER(sz), C.POINTER(sz)]
    L.pcxb_circular_create.argtypes = [sz, C.POINTER(vp), C.POINTER(sz)]
    L.pcxb_circular_destroy.argtypes = [vp]
    L.pcxb_call_sizes.argtypes = [vp, cp, C.POINTER(sz), sz]
    L.pcxb_get_sizes.argtypes = [vp, cp, C.POINTER(sz), sz, C.POINTER(sz)]
    L.pcxb_num_ports.argtypes = [vp, i, C.POINTER(sz)]
    L.pcxb_port_info.argtypes = [vp, i, sz, cp, sz, cp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.pcxb_work_ports.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.pcxb_work.argtypes = [vp, vp, sz, C.POINTER(PcxbLabel), sz, vp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz),
                            C.POINTER(PcxbLabel), sz, C.POINTER(sz)]
    L.pcxb_call_strings.argtypes = [vp, cp, C.POINTER(cp), sz]
    L.pcxb_plant_dtype.argtypes = [vp, sz, cp]
    L.pcxb_queue_packet.argtypes = [vp, sz, vp, sz, cp, C.POINTER(PcxbLabel), sz, C.POINTER(PcxbLabel), sz]
    L.pcxb_queue_label.argtypes = [vp, sz, C.POINTER(PcxbLabel)]
    L.pcxb_work_inputs.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(PcxbLabel), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(i)]
    L.pcxb_message_count.argtypes = [vp, C.POINTER(sz)]
    L.pcxb_message_info.argtypes = [vp, sz, C.POINTER(i), cp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(i), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pcxb_message_payload.argtypes = [vp, sz, vp, sz]
    L.pcxb_message_labels.argtypes = [vp, sz, C.POINTER(PcxbLabel), sz]
    L.pcxb_messages_clear.argtypes = [vp]
    if module == "comms":
        _blib = L
    else:
        _mlibs[module] = L
    return L


def _check(rc):
    _check_in("comms", rc)


def _check_in(module, rc):
    if rc == 0:
        return
    msg = load(module).pcxb_last_error().decode("utf-8", "replace")
    if rc == _lib.ERR_ARG:
        raise _lib.InvalidArgument(rc, msg)
    if rc == _lib.ERR_UNSUPPORTED:
        raise _lib.Unsupported(rc, msg)
    raise _lib.PcxError(rc, msg)


def registry_paths():
    L = load()
    return sorted(L.pcxb_registry_path(i).decode() for i in range(L.pcxb_registry_count()))


def registry_arity(path, module="comms"):
    """how many arguments the factory registered at `path` takes (-1: no such path)"""
    return int(load(module).pcxb_registry_arity(path.encode()))


def module_registry_paths(module):
    """the registry of one module library (registry_paths() is the "comms" module's)"""
    L = load(module)
    return sorted(L.pcxb_registry_path(i).decode() for i in range(L.pcxb_registry_count()))


class Label:
    """(id, index, width, data) -- data is None, an int (size_t), a float or a str."""

    def __init__(self, id, index, data=None, width=1):
        self.id, self.index, self.data, self.width = id, int(index), data, int(width)

    def __repr__(self):
        return "Label(%r, index=%d, data=%r, width=%d)" % (self.id, self.index, self.data, self.width)

    def __eq__(self, o):
        return (self.id, self.index, self.data, self.width) == (o.id, o.index, o.data, o.width)

    def _to_c(self, c):
        c.id = self.id.encode()
        c.index, c.width = self.index, self.width
        if self.data is None:
            c.kind = NONE
        elif isinstance(self.data, bool) or isinstance(self.data, (int, np.integer)):
            c.kind, c.uval = SIZE, int(self.data)
        elif isinstance(self.data, float):
            c.kind, c.dval = DOUBLE, self.data
        else:
            c.kind, c.sval = STRING, str(self.data).encode()

    @staticmethod
    def _from_c(c):
        data = None
        if c.kind == SIZE:
            data = int(c.uval)
        elif c.kind == DOUBLE:
            data = float(c.dval)
        elif c.kind == STRING:
            data = c.sval.decode()
        return Label(c.id.decode(), c.index, data, c.width)


class Message:
    """a Packet a block posted: the metadata "index", "position" (the raw double) and "level" (None where the key is absent), the
    payload's type name, its bytes and its labels (indices in elements of the payload)"""

    def __init__(self, index, position, level, dtype, payload, labels):
        self.index, self.position, self.level, self.dtype, self.payload, self.labels = index, position, level, dtype, payload, labels

    def __repr__(self):
        return "Message(index=%r, position=%r, level=%r, dtype=%r, %d bytes, %r)" % (self.index, self.position, self.level, self.dtype,
                                                                                     self.payload.size, self.labels)


class Block:
    def __init__(self, path, dtype, *args, dimension=1, module="comms"):
        self._module = module
        L = load(self._module)
        self.path = path
        self.dtype = dtype
        sarg, nbins, inverse = None, 0, 0
        if path.endswith("fir_filter") or path.endswith("/arithmetic") or path.endswith("fm_demod_chain"):
            sarg = (args[0] if args else "").encode()     # tapsType resp. operation
        elif path == "/comms/fft":
            nbins, inverse = int(args[0]), int(bool(args[1])) if len(args) > 1 else 0
        self._h = C.c_void_p()
        if module in ("logic", "math"):   # factories with an operation, a constant, a channel count, a shift size, a base, an exponent or a root: pcxb_make_args
            fargs = (PcxbArg * max(1, len(args)))(*[_factory_arg(a) for a in args])
            _check_in(self._module, L.pcxb_make_args(path.encode(), (dtype or "").encode(), dimension, fargs, len(args), C.byref(self._h)))
        else:
            _check_in(self._module, L.pcxb_make(path.encode(), (dtype or "").encode(), dimension, sarg, nbins, inverse, C.byref(self._h)))
        self._slots = []          # blocks wired to this one's signals: kept alive as long as it can emit
        if path.endswith("fir_designer"):     # no stream ports: a signal source only
            self.in_dtype = self.out_dtype = None
            self.in_dim = self.out_dim = 0
            return
        nin = C.c_size_t()
        _check_in(self._module, L.pcxb_num_ports(self._h, 0, C.byref(nin)))
        if nin.value == 0:                    # a source: driven through work_ports with no inputs
            self.in_dtype, self.in_dim = None, 0
            self.out_dtype, self.out_dim, _ = self._port(1)
            return
        self.in_dtype, self.in_dim, _ = self._port(0)
        nout = C.c_size_t()
        _check_in(self._module, L.pcxb_num_ports(self._h, 1, C.byref(nout)))
        if nout.value == 0:                   # a sink (/comms/signal_probe): driven through work_ports with no outputs
            self.out_dtype, self.out_dim = None, 0
            return
        self.out_dtype, self.out_dim, _ = self._port(1)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load(self._module).pcxb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _port(self, is_output):
        name = C.create_string_buffer(64)
        dim, nbytes = C.c_size_t(), C.c_size_t()
        _check_in(self._module, load(self._module).pcxb_port_dtype(self._h, is_output, name, 64, C.byref(dim), C.byref(nbytes)))
        return name.value.decode(), dim.value, nbytes.value

    # ---- registered calls ----
    def call(self, name, *args):
        L, n = load(self._module), name.encode()
        if name in ("setTaps", "setMap"):       # setMap: a symbol map, real or complex, as doubles (an int64 value beyond 2^53 needs the C ABI)
            t = np.asarray(args[0])
            cplx = np.iscomplexobj(t)
            flat = np.ascontiguousarray(t.astype(np.complex128)).view(np.float64) if cplx else np.ascontiguousarray(t.astype(np.float64))
            return _check_in(self._module, L.pcxb_call_taps(self._h, n, flat.ctypes.data_as(C.c_void_p), t.size, int(cplx)))
        if name in ("getTaps", "getMap"):
            cplx = bool(args[0]) if args else False
            buf = np.zeros(1 << 16, np.float64)
            cnt = C.c_size_t()
            _check_in(self._module, L.pcxb_get_taps(self._h, n, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(cnt), int(cplx)))
            return buf[:2 * cnt.value].view(np.complex128).copy() if cplx else buf[:cnt.value].copy()
        if name in ("setWindowArgs", "setFrequencies"):      # std::vector<double>
            flat = np.ascontiguousarray(np.asarray(args[0], dtype=np.float64))
            return _check_in(self._module, L.pcxb_call_taps(self._h, n, flat.ctypes.data_as(C.c_void_p), flat.size, 0))
        if name == "windowArgs":
            buf, cnt = np.zeros(64, np.float64), C.c_size_t()
            _check_in(self._module, L.pcxb_get_taps(self._h, n, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(cnt), 0))
            return buf[:cnt.value].copy()
        if name in ("setPreload", "setDevices"):
            v = (C.c_size_t * max(1, len(args[0])))(*[int(a) for a in args[0]])
            return _check_in(self._module, L.pcxb_call_sizes(self._h, n, v, len(args[0])))
        if name in ("preload", "getDevices"):
            v, cnt = (C.c_size_t * 64)(), C.c_size_t()
            _check_in(self._module, L.pcxb_get_sizes(self._h, n, v, 64, C.byref(cnt)))
            return [int(v[k]) for k in range(cnt.value)]
        if name == "setIdsList":                # std::vector<std::string>
            v = (C.c_char_p * max(1, len(args[0])))(*[str(a).encode() for a in args[0]])
            return _check_in(self._module, L.pcxb_call_strings(self._h, n, v, len(args[0])))
        if name in ("getNumPoints", "getNumWindows", "getPosition") and not args:
            v = C.c_size_t()
            _check_in(self._module, L.pcxb_get_size(self._h, n, C.byref(v)))
            return v.value
        if name in ("getAlignment", "getHoldOff", "getSource") and not args:      # (the last two are bool in the reference, WaveTrigger.cpp:273, :284)
            v = C.c_int()
            _check_in(self._module, L.pcxb_get_bool(self._h, n, C.byref(v)))
            return bool(v.value)
        if name in ("getEventRate", "getLevel") and not args:
            v = C.c_double()
            _check_in(self._module, L.pcxb_get_double(self._h, n, C.byref(v)))
            return v.value
        if name in ("setPoly", "setSeed"):      # int64_t, negative values included
            v = int(args[0])
            return _check_in(self._module, L.pcxb_call_int64(self._h, n, v - (1 << 64) if v >= (1 << 63) else v))
        if name in ("poly", "seed") and not args:
            v = C.c_int64()
            _check_in(self._module, L.pcxb_get_int64(self._h, n, C.byref(v)))
            return v.value
        if name in ("setOffset", "setAmplitude"):       # std::complex<double>
            v = complex(args[0])
            return _check_in(self._module, L.pcxb_call_complex(self._h, n, v.real, v.imag))
        if name in ("getOffset", "getAmplitude"):
            re, im = C.c_double(), C.c_double()
            _check_in(self._module, L.pcxb_get_complex(self._h, n, C.byref(re), C.byref(im)))
            return complex(re.value, im.value)
        if name in ("setActivationLevel", "setDeactivationLevel"):      # one element of the stream type: an integer level keeps its 64 bits
            if str(self.dtype).startswith("float"):
                return _check_in(self._module, L.pcxb_call_double(self._h, n, float(args[0])))
            return _check_in(self._module, L.pcxb_call_int64(self._h, n, int(args[0])))
        if name in ("getActivationLevel", "getDeactivationLevel"):
            if str(self.dtype).startswith("float"):
                v = C.c_double()
                _check_in(self._module, L.pcxb_get_double(self._h, n, C.byref(v)))
            else:
                v = C.c_int64()
                _check_in(self._module, L.pcxb_get_int64(self._h, n, C.byref(v)))
            return v.value
        if name == "setConstant":       # one element of the stream type (the logic module): complex, float, or an integer that keeps its 64 bits
            if str(self.dtype).startswith("complex_"):
                v = complex(args[0])
                return _check_in(self._module, L.pcxb_call_complex(self._h, n, v.real, v.imag))
            if str(self.dtype).startswith("float"):
                return _check_in(self._module, L.pcxb_call_double(self._h, n, float(args[0])))
            v = int(args[0])
            return _check_in(self._module, L.pcxb_call_int64(self._h, n, v - (1 << 64) if v >= (1 << 63) else v))
        if name == "constant" and not args:
            if str(self.dtype).startswith("complex_"):
                re, im = C.c_double(), C.c_double()
                _check_in(self._module, L.pcxb_get_complex(self._h, n, C.byref(re), C.byref(im)))
                return complex(re.value, im.value)
            if str(self.dtype).startswith("float"):
                v = C.c_double()
                _check_in(self._module, L.pcxb_get_double(self._h, n, C.byref(v)))
                return v.value
            v = C.c_int64()
            _check_in(self._module, L.pcxb_get_int64(self._h, n, C.byref(v)))
            return v.value + (1 << 64) if v.value < 0 and str(self.dtype).startswith("uint") else v.value
        if name == "value" and not args:        # /comms/signal_probe: a double on a real stream, a std::complex<double> on a complex one
            re, im = C.c_double(), C.c_double()
            _check_in(self._module, L.pcxb_get_complex(self._h, n, C.byref(re), C.byref(im)))
            return complex(re.value, im.value) if str(self.dtype).startswith("complex_") else re.value
        if name.startswith("probe") and not args:       # a registerProbe slot: emits "<name>Triggered" and returns nothing
            return self.call_slot(name)
        if name in ("setBase", "setExponent", "setRoot"):       # one value of the stream type (the math module)
            return _check_in(self._module, L.pcxb_call_double(self._h, n, float(args[0])))
        if name in ("base", "exponent", "root") and not args:
            v = C.c_double()
            _check_in(self._module, L.pcxb_get_double(self._h, n, C.byref(v)))
            return v.value
        if name == "setPreamble" and str(self.dtype).startswith("complex_"):      # /comms/frame_insert: std::vector<std::complex<T>>
            t = np.ascontiguousarray(np.asarray(args[0]).astype(np.complex128).reshape(-1))
            return _check_in(self._module, L.pcxb_call_taps(self._h, n, t.view(np.float64).ctypes.data_as(C.c_void_p), t.size, 1))
        if name == "getPreamble" and str(self.dtype).startswith("complex_"):
            buf, cnt = np.zeros(1 << 16, np.float64), C.c_size_t()
            _check_in(self._module, L.pcxb_get_taps(self._h, n, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(cnt), 1))
            return buf[:2 * cnt.value].view(np.complex128).copy()
        if name == "setPreamble":               # std::vector<unsigned char>
            v = np.ascontiguousarray(np.asarray(args[0], dtype=np.uint8).reshape(-1))
            return _check_in(self._module, L.pcxb_call_bytes(self._h, n, v.ctypes.data_as(C.c_void_p) if v.size else None, v.size))
        if name == "getPreamble":
            buf, cnt = np.zeros(1 << 16, np.uint8), C.c_size_t()
            _check_in(self._module, L.pcxb_get_bytes(self._h, n, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(cnt)))
            return [int(b) for b in buf[:cnt.value]]
        if not args:   # getter
            if name in ("getThreshold", "getDecimation", "getInterpolation", "getNumInlineBuffers", "numTaps", "getShardPasses", "getDevice", "getPortSlabBytes",
                        "getAverageSize", "getCascadeSize", "getLookahead", "getSymbols", "getModulus", "getPaddingSize", "getSymbolWidth", "getHeaderId", "shiftSize",
                        "getWindow", "getDataWidth"):
                v = C.c_size_t()
                _check_in(self._module, L.pcxb_get_size(self._h, n, C.byref(v)))
                return v.value
            if name in ("getWaitTaps",):
                v = C.c_int()
                _check_in(self._module, L.pcxb_get_bool(self._h, n, C.byref(v)))
                return bool(v.value)
            if name in ("getPhase", "getFactor", "sampleRate", "frequencyLower", "frequencyUpper", "bandwidthTrans", "alpha",
                        "stopDB", "passDB", "gain", "getAttack", "getRelease", "getFrequency", "getSampleRate", "getResolution", "getMean", "getB", "getRate", "getInputThreshold"):
                v = C.c_double()
                _check_in(self._module, L.pcxb_get_double(self._h, n, C.byref(v)))
                return v.value
            s = C.create_string_buffer(128)
            _check_in(self._module, L.pcxb_get_string(self._h, n, s, 128))
            return s.value.decode()
        a = args[0]
        if isinstance(a, bool):
            return _check_in(self._module, L.pcxb_call_bool(self._h, n, int(a)))
        if isinstance(a, (int, np.integer)):
            return _check_in(self._module, L.pcxb_call_size(self._h, n, int(a)))
        if isinstance(a, float):
            return _check_in(self._module, L.pcxb_call_double(self._h, n, a))
        return _check_in(self._module, L.pcxb_call_string(self._h, n, str(a).encode()))

    def call_slot(self, name):
        """a registered call without an argument whose result is not wanted (a slot such as "probeValue")"""
        _check_in(self._module, load(self._module).pcxb_call_void(self._h, name.encode()))

    def reserve(self):
        """the reserve input 0 stands at now (None: none asked for)"""
        r = C.c_size_t()
        _check_in(self._module, load(self._module).pcxb_input_reserve(self._h, C.byref(r)))
        return None if r.value == _SIZE_MAX else r.value

    def calls(self):
        """{name: number of arguments} of the calls the block registered"""
        L = load(self._module)
        n = C.c_size_t()
        _check_in(self._module, L.pcxb_call_count(self._h, C.byref(n)))
        out = {}
        buf = C.create_string_buffer(128)
        for i in range(n.value):
            _check_in(self._module, L.pcxb_call_name(self._h, i, buf, len(buf)))
            out[buf.value.decode()] = int(L.pcxb_call_arity(self._h, buf.value))
        return out

    def activate(self):
        _check_in(self._module, load(self._module).pcxb_activate(self._h))

    def deactivate(self):
        _check_in(self._module, load(self._module).pcxb_deactivate(self._h))

    def connect_signal(self, signal, dst, slot):
        """Topology::connect(self, signal, dst, slot): later emissions call dst's registered `slot` synchronously."""
        _check_in(self._module, load(self._module).pcxb_connect_signal(self._h, signal.encode(), dst._h, slot.encode()))
        self._slots.append(dst)

    def buffer_manager(self, is_output):
        name = C.create_string_buffer(64)
        sz = C.c_size_t()
        _check_in(self._module, load(self._module).pcxb_buffer_manager(self._h, int(is_output), name, 64, C.byref(sz)))
        return name.value.decode(), sz.value

    def port_buffer(self, is_output, shape, dtype):
        """The next port buffer from the manager the block handed the scheduler (pcxb_acquire_buffer), as a numpy
        array of `shape` / `dtype` over the slab -- page-locked for the device-backed blocks.  Returns (array, pinned)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p, sz, pin = C.c_void_p(), C.c_size_t(), C.c_int()
        _check_in(self._module, load(self._module).pcxb_acquire_buffer(self._h, int(is_output), nbytes, C.byref(p), C.byref(sz), C.byref(pin)))
        arr = np.ctypeslib.as_array((C.c_char * nbytes).from_address(p.value)).view(dtype).reshape(shape)
        return arr, bool(pin.value)

    def link_buffer(self, downstream, nbytes):
        """The buffer a scheduler would plant on the edge self.output(0) -> downstream.input(0) (pcxb_link_buffer).
        Returns (address, kind): kind 2 = device memory (two blocks of this module), 1 = page-locked host, 0 = pageable."""
        p, sz, kind = C.c_void_p(), C.c_size_t(), C.c_int()
        _check_in(self._module, load(self._module).pcxb_link_buffer(self._h, downstream._h, nbytes, C.byref(p), C.byref(sz), C.byref(kind)))
        return p.value, kind.value

    def work_raw(self, in_ptr, in_elems, out_ptr, out_elems, labels=()):
        """One work() call on raw buffer addresses (host or device memory).  Returns (consumed, produced, reserve)."""
        labs, posted = (PcxbLabel * max(1, len(labels)))(), (PcxbLabel * 64)()
        for i, l in enumerate(labels):
            l._to_c(labs[i])
        c, p, r, npost = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        _check_in(self._module, load(self._module).pcxb_work(self._h, C.c_void_p(in_ptr), in_elems, labs, len(labels), C.c_void_p(out_ptr), out_elems, C.byref(c), C.byref(p),
                                C.byref(r), posted, 64, C.byref(npost)))
        return c.value, p.value, (None if r.value == _SIZE_MAX else r.value)

    def work_loop(self, in_ptr, in_elems, out_ptr, out_elems, reps):
        """pcxb_work_loop: `reps` work() calls on the same buffers from native code.  Returns (seconds, consumed, produced) of the loop /
        its last call."""
        t, c, p = C.c_double(), C.c_size_t(), C.c_size_t()
        _check_in(self._module, load(self._module).pcxb_work_loop(self._h, C.c_void_p(in_ptr), in_elems, C.c_void_p(out_ptr), out_elems, reps, C.byref(t), C.byref(c), C.byref(p)))
        return t.value, c.value, p.value

    def initial_reserve(self):
        r = C.c_size_t()
        load(self._module).pcxb_initial_reserve(self._h, C.byref(r))
        return None if r.value == _SIZE_MAX else r.value

    def ports(self, is_output):
        """[(name, dtype name, dimension, bytes per element, preloaded elements)] -- indexed ports first."""
        L = load(self._module)
        cnt = C.c_size_t()
        _check_in(self._module, L.pcxb_num_ports(self._h, int(is_output), C.byref(cnt)))
        out = []
        for k in range(cnt.value):
            nm, dt = C.create_string_buffer(64), C.create_string_buffer(64)
            dim, nb, pre = C.c_size_t(), C.c_size_t(), C.c_size_t()
            _check_in(self._module, L.pcxb_port_info(self._h, int(is_output), k, nm, 64, dt, 64, C.byref(dim), C.byref(nb), C.byref(pre)))
            out.append((nm.value.decode(), dt.value.decode(), dim.value, nb.value, pre.value))
        return out

    def work_ports(self, ins, out_elems, inline=False):
        """One work() call with a buffer planted on every port (ins: one array per input port, out_elems:
        room per output port).  inline=True plants input 0's buffer as output 0 (the buffer forwarding the
        reference's setReadBeforeWrite enables).  Returns (outs trimmed to produced, consumed, produced)."""
        L = load(self._module)
        ip, op = self.ports(0), self.ports(1)
        xs = [np.ascontiguousarray(as_pairs(x)) for x in ins]
        if isinstance(out_elems, int):
            out_elems = [out_elems] * len(op)
        ys = []
        for (nm, dt, dim, nb, _), ne in zip(op, out_elems):
            scalar, cplx = parse_dtype(dt)
            ys.append(np.zeros([ne * dim] + ([2] if cplx else []), dtype=NP_SCALAR[scalar]))
        if inline:
            ys[0] = xs[0]
        in_ptrs = (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])
        in_n = (C.c_size_t * len(xs))(*[x.shape[0] // p[2] for x, p in zip(xs, ip)])
        out_ptrs = (C.c_void_p * len(ys))(*[y.ctypes.data for y in ys])
        out_n = (C.c_size_t * len(ys))(*[int(n) for n in out_elems])
        cons, prod = (C.c_size_t * len(xs))(), (C.c_size_t * len(ys))()
        _check_in(self._module, L.pcxb_work_ports(self._h, len(xs), in_ptrs, in_n, len(ys), out_ptrs, out_n, cons, prod))
        produced = [int(v) for v in prod]
        return [y[:p * port[2]] for y, p, port in zip(ys, produced, op)], [int(v) for v in cons], produced

    def work_ports_raw(self, in_ptrs, in_elems, out_ptrs, out_elems):
        """pcxb_work_ports on raw buffer addresses (host or device memory), one per port; a block without inputs takes two empty lists.
        Returns (consumed, produced), one entry per port."""
        ins, outs = (C.c_void_p * len(in_ptrs))(*in_ptrs), (C.c_void_p * len(out_ptrs))(*out_ptrs)
        nin, nout = (C.c_size_t * len(in_ptrs))(*in_elems), (C.c_size_t * len(out_ptrs))(*out_elems)
        cons, prod = (C.c_size_t * len(in_ptrs))(), (C.c_size_t * len(out_ptrs))()
        _check_in(self._module, load(self._module).pcxb_work_ports(self._h, len(in_ptrs), ins, nin, len(out_ptrs), outs, nout, cons, prod))
        return [int(v) for v in cons], [int(v) for v in prod]

    # ---- messages and packets (/comms/wave_trigger) ----
    def plant_dtype(self, port, dtype):
        """the type the buffers planted on input `port` carry, for a port that has none of its own ("" or None: unspecified)"""
        _check_in(self._module, load(self._module).pcxb_plant_dtype(self._h, port, (dtype or "").encode()))

    @staticmethod
    def _labels_to_c(labels):
        labs = (PcxbLabel * max(1, len(labels)))()
        for i, l in enumerate(labels):
            l._to_c(labs[i])
        return labs

    def queue_packet(self, port, payload, dtype, labels=(), metadata=None):
        """a Packet on input `port`: payload a numpy array (its bytes are copied), dtype the payload's type name ("" or None: none),
        labels in elements of the payload, metadata {key: int, float or str}"""
        raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        meta = [Label(k, 0, v) for k, v in (metadata or {}).items()]
        _check_in(self._module, load(self._module).pcxb_queue_packet(self._h, port, raw.ctypes.data_as(C.c_void_p) if raw.size else None, raw.size,
                                                                     (dtype or "").encode(), self._labels_to_c(labels), len(labels),
                                                                     self._labels_to_c(meta), len(meta)))

    def queue_label(self, port, label):
        """a Label as a message on input `port`"""
        _check_in(self._module, load(self._module).pcxb_queue_label(self._h, port, self._labels_to_c([label])))

    def work_inputs(self, in_ptrs, in_elems, labels=None):
        """One work() call over the indexed input ports on raw buffer addresses (host or device memory): in_elems[i] elements of port
        i's type (of the planted type on a port without one), labels[i] the port's labels in the port's own units (bytes on a port
        without a type).  Returns (consumed, reserve, yielded): per port, in the port's own units, reserve None where none was asked
        for.  What the block posted stays queued: messages()."""
        nin = len(in_ptrs)
        labels = labels or [()] * nin
        flat = [l for port in labels for l in port]
        ins, ne = (C.c_void_p * max(1, nin))(*in_ptrs), (C.c_size_t * max(1, nin))(*in_elems)
        nl = (C.c_size_t * max(1, nin))(*[len(p) for p in labels])
        cons, res, y = (C.c_size_t * max(1, nin))(), (C.c_size_t * max(1, nin))(), C.c_int()
        _check_in(self._module, load(self._module).pcxb_work_inputs(self._h, nin, ins, ne, self._labels_to_c(flat), nl, cons, res, C.byref(y)))
        return [int(v) for v in cons][:nin], [None if v == _SIZE_MAX else int(v) for v in res][:nin], bool(y.value)

    def messages(self, clear=True):
        """what output 0 holds, oldest first: ("packet", Message) / ("label", Label) / ("other", None).  A Message has index (the
        metadata "index", or None), position (the raw double, or None), level, dtype, payload (uint8) and labels."""
        L = load(self._module)
        n = C.c_size_t()
        _check_in(self._module, L.pcxb_message_count(self._h, C.byref(n)))
        out = []
        for k in range(n.value):
            kind, dt, nb, nl, has = C.c_int(), C.create_string_buffer(64), C.c_size_t(), C.c_size_t(), C.c_int()
            idx, pos, lev = C.c_int64(), C.c_double(), C.c_double()
            _check_in(self._module, L.pcxb_message_info(self._h, k, C.byref(kind), dt, 64, C.byref(nb), C.byref(nl), C.byref(has), C.byref(idx),
                                                        C.byref(pos), C.byref(lev)))
            labs = (PcxbLabel * max(1, nl.value))()
            if kind.value != MSG_OTHER:
                _check_in(self._module, L.pcxb_message_labels(self._h, k, labs, nl.value))
            labels = [Label._from_c(labs[j]) for j in range(nl.value)]
            if kind.value == MSG_LABEL:
                out.append(("label", labels[0]))
            elif kind.value == MSG_PACKET:
                payload = np.zeros(nb.value, np.uint8)
                if nb.value:
                    _check_in(self._module, L.pcxb_message_payload(self._h, k, payload.ctypes.data_as(C.c_void_p), nb.value))
                out.append(("packet", Message(idx.value if has.value & HAS_INDEX else None, pos.value if has.value & HAS_POSITION else None,
                                              lev.value if has.value & HAS_LEVEL else None, dt.value.decode(), payload, labels)))
            else:
                out.append(("other", None))
        if clear:
            _check_in(self._module, L.pcxb_messages_clear(self._h))
        return out

    def work(self, inbuf, out_elems, labels=(), outbuf=None, label_cap=64):
        """One work() call.  Returns (out[:produced], consumed, produced, reserve, posted_labels).
        outbuf: write into this array (e.g. a slab from port_buffer) instead of a fresh one.
        label_cap: how many posted labels come back at most (a correlator can post one per symbol)."""
        x = as_pairs(inbuf)
        scalar, cplx = parse_dtype(self.out_dtype)
        shape = [out_elems * self.out_dim] + ([2] if cplx else [])
        if outbuf is None:
            y = np.zeros(shape, dtype=NP_SCALAR[scalar])
        else:
            y = outbuf
            assert y.flags.c_contiguous and y.dtype == NP_SCALAR[scalar] and y.size >= int(np.prod(shape))
        in_elems = x.shape[0] // self.in_dim
        labs = (PcxbLabel * max(1, len(labels)))()
        for i, l in enumerate(labels):
            l._to_c(labs[i])
        posted = (PcxbLabel * label_cap)()
        c, p, r, npost = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        _check_in(self._module, load(self._module).pcxb_work(self._h, x.ctypes.data_as(C.c_void_p), in_elems, labs, len(labels),
                                y.ctypes.data_as(C.c_void_p), out_elems, C.byref(c), C.byref(p), C.byref(r),
                                posted, label_cap, C.byref(npost)))
        reserve = None if r.value == _SIZE_MAX else r.value
        return (y[:p.value * self.out_dim], c.value, p.value, reserve,
                [Label._from_c(posted[i]) for i in range(min(npost.value, label_cap))])


class CircularBuffer:
    """The framework's "circular" buffer (pcxb_circular_create): `size` bytes of PAGEABLE shared memory mapped twice back to back --
    view(off, n) for any off < size and n <= size is contiguous, running across the wrap into the second mapping.  What Pothos hands a
    block that asks for BufferManager::make("circular") (filter/FIRFilter.cpp:196-199).  close() it after the blocks that saw it."""

    def __init__(self, nbytes):
        p, n = C.c_void_p(), C.c_size_t()
        _check(load().pcxb_circular_create(nbytes, C.byref(p), C.byref(n)))
        self.base, self.size = p.value, n.value

    def view(self, offset, nbytes, dtype=np.uint8):
        assert 0 <= offset < self.size and 0 <= nbytes <= self.size
        return np.ctypeslib.as_array((C.c_char * nbytes).from_address(self.base + offset)).view(dtype)

    def close(self):
        if getattr(self, "base", None):
            _check(load().pcxb_circular_destroy(C.c_void_p(self.base)))
            self.base = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make(path, dtype=None, *args, dimension=1, module="comms"):
    """BlockRegistry::make(path, dtype, *args) in the registry of `module` (MODULES)."""
    return Block(path, dtype, *args, dimension=dimension, module=module)
