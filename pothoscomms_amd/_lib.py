"""ctypes binding of libpcx_hip.so (include/pcx.h).

The library is the product's only compute path.  If it is missing or fails to
load, importing the binding raises -- there is no CPU fallback anywhere in
this package (the CPU oracle under oracle/ is test infrastructure only).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpcx_hip.so")

# pcx_scalar
F64, F32, I64, I32, I16, I8, U64, U32, U16, U8 = range(10)   # unsigned: pcx_arith*, pcx_arith_const*, pcx_compare*, pcx_bitwise*, pcx_bitshift* only
ARITH_ADD, ARITH_SUB, ARITH_MUL, ARITH_DIV = range(4)
CMP_GT, CMP_LT, CMP_GE, CMP_LE, CMP_EQ, CMP_NE = range(6)            # pcx_cmp_op
BIT_NOT, BIT_AND, BIT_OR, BIT_XOR = range(4)                         # pcx_bit_op
ARITHK_X_ADD_K, ARITHK_X_SUB_K, ARITHK_K_SUB_X, ARITHK_X_MUL_K, ARITHK_X_DIV_K, ARITHK_K_DIV_X = range(6)     # pcx_arithk_op
# pcx_math_fn: name -> code; the last four take a parameter (pcx_mathfn_param)
MATH_FN = dict(zip(("EXP", "EXP2", "EXP10", "EXPM1", "LOG", "LOG2", "LOG10", "LOG1P", "SQRT", "CBRT", "RSQRT", "SINC", "SIGMOID"), range(13)))
MATH_TRIG_OPS = ("COS", "SIN", "TAN", "SEC", "CSC", "COT", "ACOS", "ASIN", "ATAN", "ASEC", "ACSC", "ACOT",
                 "COSH", "SINH", "TANH", "SECH", "CSCH", "COTH", "ACOSH", "ASINH", "ATANH", "ASECH", "ACSCH", "ACOTH")
MATH_FN.update(zip(MATH_TRIG_OPS, range(16, 40)))
MATH_FN.update(zip(("EXPN", "LOGN", "POW", "NTH_ROOT"), range(48, 52)))
MATH_FN_PARAM = ("EXPN", "LOGN", "POW", "NTH_ROOT")
# pcx_spec_fn: name -> code (pcx_specfn); beta and modf have calls of their own
SPEC_FN = dict(zip(("GAMMA", "LNGAMMA", "ERF", "ERFC"), range(4)))
# pcx_status
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_STATE = 0, -1, -2, -3, -4
# pcx_fir_algo
FIR_AUTO, FIR_DIRECT, FIR_OLS_FFT, FIR_EXACT = 0, 1, 2, 3
# pcx_fir_get_last_plan: PCX_FIR_PLAN_*, in the order of their values
FIR_PLANS = ("NONE", "CF32_OLS4096", "CF32_OLS4096_GATED", "CF32_UPOLS", "CF32_DECIM", "CF32_INTERP", "CF32_OLS4096_ROWS", "CF32_POLY",
             "F32_OLS4096", "F32_UPOLS", "F32_OLS4096_ROWS", "UPOLS_ROWS", "UPOLS_DECIM", "CF64_OLS", "CF64_OLS_ROWS", "REAL64_OLS",
             "REAL64_OLS_ROWS", "CF32_DIRECT_TILE", "DOT2", "SLIDE", "GENERIC")
IIR_SCAN, IIR_SERIAL = 0, 1          # pcx_iir_get_plan
# pcx_fft_get_plan: PCX_FFT_PLAN_*, in the order of the handle's kinds
FFT_PLANS = ("IDENTITY", "R16_4096", "R16", "POW2", "Q15_POW2", "Q15_GLOBAL", "MIXED", "SMOOTH", "FOURSTEP", "FOURSTEP_SHORT", "BLUESTEIN")
SCR_ADDITIVE, SCR_MULTIPLICATIVE = 0, 1     # pcx_scrambler_set_mode
SCR_SCAN, SCR_SERIAL = 0, 1          # pcx_scrambler_get_plan
PRE_PLANES, PRE_BYTES = 0, 1         # pcx_preamble_get_plan
DIFF_SCAN, DIFF_SERIAL = 0, 1        # pcx_diffcode_get_plan
REPACK_BITS_TO_SYMBOLS, REPACK_SYMBOLS_TO_BITS, REPACK_BYTES_TO_SYMBOLS, REPACK_SYMBOLS_TO_BYTES = 0, 1, 2, 3      # pcx_repack_create
WAVE_CONST, WAVE_SINE, WAVE_RAMP, WAVE_SQUARE = 0, 1, 2, 3                       # pcx_waveform_table
NOISE_UNIFORM, NOISE_NORMAL, NOISE_LAPLACE, NOISE_POISSON = 0, 1, 2, 3           # pcx_noise_table
NOISE_ENTRIES = 4096
PROBE_VALUE, PROBE_RMS, PROBE_MEAN = 0, 1, 2                                     # pcx_probe_set_mode
TRIGGER_POS, TRIGGER_NEG, TRIGGER_LEVEL = 0, 1, 2                                # pcx_trigger_set_slope
TRIGGER_MAX_PORTS = 16
FRAME_OTHER, FRAME_START, FRAME_END = 0, 1, 2                                   # pcx_frame_event.kind
SEG_INPUT, SEG_POOL, SEG_HEADER, SEG_ZERO = 0, 1, 2, 3                           # pcx_frame_segment.kind
FRAME_HEADER_BITS = 58


class PcxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("pcx status %d: %s" % (status, msg))
        self.status = status


class InvalidArgument(PcxError, ValueError):
    """Mirror of Pothos::InvalidArgumentException at the block boundary."""


class Unsupported(PcxError, NotImplementedError):
    """Valid in the reference, not implemented on the device path."""


# pcx_q_frac / pcx_q_to / pcx_q_from
Q_FRAC_HALF_Q, Q_FRAC_HALF_ELEM = 0, 1
Q_TRUNCATE, Q_NEAREST = 0, 1
Q_FLOOR, Q_TOWARD_ZERO, Q_ROUND = 0, 1, 2


class QFormat(C.Structure):
    """pcx_qformat: the floatToQ / fromQ reading of the integer element types (include/pcx.h)."""
    _fields_ = [("frac", C.c_int), ("float_to_q", C.c_int), ("from_q", C.c_int)]


def qformat_ptr(q):
    """None -> NULL (the process-wide reading); a QFormat or a (frac, float_to_q, from_q) triple -> pointer to a pcx_qformat"""
    if q is None:
        return None
    if not isinstance(q, QFormat):
        q = QFormat(*[int(v) for v in q])
    return C.byref(q)


class FrameEvent(C.Structure):
    """pcx_frame_event: a label of a framer call (include/pcx.h)."""
    _fields_ = [("index", C.c_uint64), ("width", C.c_uint64), ("kind", C.c_uint32), ("length", C.c_uint32)]


class FrameSegment(C.Structure):
    """pcx_frame_segment: one run of a framer call's output, in elements."""
    _fields_ = [("dst", C.c_uint64), ("src", C.c_uint64), ("kind", C.c_uint32), ("reserved", C.c_uint32)]


class FramePlan(C.Structure):
    """pcx_frame_plan: what a framer call consumes and produces."""
    _fields_ = [("consumed", C.c_uint64), ("used_events", C.c_uint64), ("out_len", C.c_uint64), ("n_segments", C.c_uint64),
                ("n_headers", C.c_uint64), ("cut", C.c_int)]


class FsyncLabel(C.Structure):
    """pcx_fsync_label: a label a frame sync call posts on its output."""
    _fields_ = [("kind", C.c_uint32), ("reserved", C.c_uint32), ("index", C.c_uint64), ("width", C.c_uint64), ("length", C.c_uint64),
                ("value", C.c_double)]


class FsyncResult(C.Structure):
    """pcx_fsync_result: what a frame sync call did and the state it leaves."""
    _fields_ = [("consumed", C.c_uint64), ("produced", C.c_uint64), ("reserve", C.c_uint64), ("n_labels", C.c_uint32), ("reserved", C.c_uint32),
                ("labels", FsyncLabel * 3), ("remaining", C.c_uint64), ("phase", C.c_double), ("phase_inc", C.c_double), ("scale", C.c_double),
                ("delta_fc", C.c_double), ("phase_off", C.c_double), ("max_peak", C.c_uint64), ("count_since_max", C.c_uint64)]


class TriggerHit(C.Structure):
    """pcx_trigger_hit: what a wave trigger search leaves, 24 bytes."""
    _fields_ = [("i", C.c_uint64), ("y0", C.c_float), ("y1", C.c_float), ("found", C.c_uint64)]


_vp, _sz, _i, _d = C.c_void_p, C.c_size_t, C.c_int, C.c_double
_psz = C.POINTER(C.c_size_t)

# name -> (restype, argtypes): every symbol include/pcx.h declares
SIGNATURES = {
    "pcx_last_error": (C.c_char_p, []),
    "pcx_version": (C.c_char_p, []),
    "pcx_device_count": (_i, [C.POINTER(_i)]),
    "pcx_set_device": (_i, [_i]),
    "pcx_get_device": (_i, [C.POINTER(_i)]),
    "pcx_dev_alloc": (_i, [C.POINTER(_vp), _sz]),
    "pcx_dev_free": (_i, [_vp]),
    "pcx_memcpy_h2d": (_i, [_vp, _vp, _sz, _vp]),
    "pcx_memcpy_d2h": (_i, [_vp, _vp, _sz, _vp]),
    "pcx_memcpy_d2d": (_i, [_vp, _vp, _sz, _vp]),
    "pcx_stream_sync": (_i, [_vp]),
    "pcx_pointer_kind": (_i, [_vp, C.POINTER(_i)]),
    "pcx_memcpy_to_host": (_i, [_vp, _vp, _sz]),
    "pcx_trace": (_i, [_i]),
    "pcx_host_alloc": (_i, [C.POINTER(_vp), _sz]),
    "pcx_host_free": (_i, [_vp]),
    "pcx_pcie_probe": (_i, [_sz, _i, C.POINTER(_d), C.POINTER(_d), C.POINTER(_d)]),
    "pcx_host_register": (_i, [_vp, _sz]),
    "pcx_host_unregister": (_i, [_vp]),
    "pcx_host_register_mapping": (_i, [_vp, _sz, _sz, C.POINTER(_vp), _psz]),
    "pcx_host_mapping_alive": (_i, [_vp, C.POINTER(_i)]),
    "pcx_host_release_range": (_i, [_vp, _sz]),
    "pcx_fill_uniform_f32_dev": (_i, [_vp, _sz, C.c_uint64, C.c_uint64, _vp]),
    "pcx_clock_probe_dev": (_i, [_vp, C.c_uint, _vp]),
    "pcx_fir_create": (_i, [_i, _i, _i, C.POINTER(_vp)]),
    "pcx_fir_destroy": (_i, [_vp]),
    "pcx_fir_set_taps": (_i, [_vp, _vp, _sz]),
    "pcx_fir_set_decimation": (_i, [_vp, _sz]),
    "pcx_fir_set_interpolation": (_i, [_vp, _sz]),
    "pcx_fir_set_algo": (_i, [_vp, _i]),
    "pcx_fir_set_qformat": (_i, [_vp, _vp]),
    "pcx_set_qformat": (_i, [_vp]),
    "pcx_get_qformat": (_i, [_vp]),
    "pcx_fir_get_geometry": (_i, [_vp, _psz, _psz]),
    "pcx_fir_last_algo": (_i, [_vp]),
    "pcx_fir_get_last_plan": (_i, [_vp, C.POINTER(_i)]),
    "pcx_fir_set_slots": (_i, [_vp, C.c_uint]),
    "pcx_fir_process": (_i, [_vp, _vp, _sz, _vp, _sz, _psz, _psz]),
    "pcx_fir_process_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _psz, _psz, _vp]),
    "pcx_fir_process_dev_gated": (_i, [_vp, _vp, _sz, _vp, _sz, _psz, _psz, _vp, C.c_uint, _vp, C.POINTER(C.c_int)]),
    "pcx_gate_signal_dev": (_i, [_vp, C.c_uint, _vp]),
    "pcx_fft_create": (_i, [_i, _sz, _i, C.POINTER(_vp)]),
    "pcx_fft_destroy": (_i, [_vp]),
    "pcx_fft_transform": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_fft_transform_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_fft_get_plan": (_i, [_vp, C.POINTER(_i), C.POINTER(_sz), C.POINTER(_sz)]),
    "pcx_freqdemod_create": (_i, [_i, C.POINTER(_vp)]),
    "pcx_freqdemod_destroy": (_i, [_vp]),
    "pcx_freqdemod_reset": (_i, [_vp]),
    "pcx_freqdemod_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_freqdemod_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_dcremoval_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "pcx_dcremoval_destroy": (_i, [_vp]),
    "pcx_dcremoval_set_sizes": (_i, [_vp, _sz, _sz]),
    "pcx_dcremoval_get_sizes": (_i, [_vp, _psz, _psz]),
    "pcx_dcremoval_reset": (_i, [_vp]),
    "pcx_dcremoval_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_dcremoval_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_envelope_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "pcx_envelope_destroy": (_i, [_vp]),
    "pcx_envelope_set_attack": (_i, [_vp, C.c_float]),
    "pcx_envelope_get_attack": (_i, [_vp, C.POINTER(C.c_float)]),
    "pcx_envelope_set_release": (_i, [_vp, C.c_float]),
    "pcx_envelope_get_release": (_i, [_vp, C.POINTER(C.c_float)]),
    "pcx_envelope_set_lookahead": (_i, [_vp, _sz]),
    "pcx_envelope_get_lookahead": (_i, [_vp, _psz]),
    "pcx_envelope_reset": (_i, [_vp]),
    "pcx_envelope_get_state": (_i, [_vp, C.POINTER(C.c_float)]),
    "pcx_envelope_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_envelope_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_envelope_get_stats": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcx_envelope_set_warmup": (_i, [_vp, _sz]),
    "pcx_iir_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "pcx_iir_destroy": (_i, [_vp]),
    "pcx_iir_set_taps": (_i, [_vp, _vp, _sz]),
    "pcx_iir_get_taps": (_i, [_vp, _vp, _sz, _psz]),
    "pcx_iir_reset": (_i, [_vp]),
    "pcx_iir_get_plan": (_i, [_vp, C.POINTER(_i), C.POINTER(_d)]),
    "pcx_iir_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_iir_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_scrambler_create": (_i, [_i, C.POINTER(_vp)]),
    "pcx_scrambler_destroy": (_i, [_vp]),
    "pcx_scrambler_set_poly": (_i, [_vp, C.c_int64]),
    "pcx_scrambler_get_poly": (_i, [_vp, C.POINTER(C.c_int64)]),
    "pcx_scrambler_set_seed": (_i, [_vp, C.c_int64]),
    "pcx_scrambler_get_seed": (_i, [_vp, C.POINTER(C.c_int64)]),
    "pcx_scrambler_set_mode": (_i, [_vp, _i]),
    "pcx_scrambler_get_mode": (_i, [_vp, C.POINTER(_i)]),
    "pcx_scrambler_get_plan": (_i, [_vp, C.POINTER(_i)]),
    "pcx_scrambler_get_geometry": (_i, [_psz, _psz, _psz, _psz]),
    "pcx_scrambler_get_state": (_i, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pcx_scrambler_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_scrambler_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_preamble_create": (_i, [C.POINTER(_vp)]),
    "pcx_preamble_destroy": (_i, [_vp]),
    "pcx_preamble_set_preamble": (_i, [_vp, _vp, _sz]),
    "pcx_preamble_get_preamble": (_i, [_vp, _vp, _sz, _psz]),
    "pcx_preamble_set_threshold": (_i, [_vp, C.c_uint]),
    "pcx_preamble_get_threshold": (_i, [_vp, C.POINTER(C.c_uint)]),
    "pcx_preamble_get_plan": (_i, [_vp, C.POINTER(_i)]),
    "pcx_preamble_get_geometry": (_i, [_psz, _psz, _psz]),
    "pcx_preamble_process": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _psz, _psz]),
    "pcx_preamble_process_dev": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp]),
    "pcx_preamble_distances": (_i, [_vp, _vp, _sz, _vp, _psz]),
    "pcx_preamble_distances_dev": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "pcx_threshold_create": (_i, [C.POINTER(_vp), _i]),
    "pcx_threshold_destroy": (_i, [_vp]),
    "pcx_threshold_set_levels": (_i, [_vp, _vp, _vp]),
    "pcx_threshold_get_levels": (_i, [_vp, _vp, _vp]),
    "pcx_threshold_reset": (_i, [_vp]),
    "pcx_threshold_get_state": (_i, [_vp, C.POINTER(_i)]),
    "pcx_threshold_set_state": (_i, [_vp, _i]),
    "pcx_threshold_get_geometry": (_i, [_psz, _psz]),
    "pcx_threshold_process": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _psz, C.POINTER(_i)]),
    "pcx_threshold_process_dev": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp]),
    "pcx_threshold_states": (_i, [_vp, _vp, _sz, _vp]),
    "pcx_threshold_states_dev": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "pcx_probe_create": (_i, [C.POINTER(_vp), _i, _i]),
    "pcx_probe_destroy": (_i, [_vp]),
    "pcx_probe_set_mode": (_i, [_vp, _i]),
    "pcx_probe_get_mode": (_i, [_vp, C.POINTER(_i)]),
    "pcx_probe_set_window": (_i, [_vp, _sz]),
    "pcx_probe_get_window": (_i, [_vp, _psz]),
    "pcx_probe_get_geometry": (_i, [_vp, _psz, _psz, _psz]),
    "pcx_probe_process": (_i, [_vp, _vp, _sz, _vp, _psz]),
    "pcx_probe_process_dev": (_i, [_vp, _vp, _sz, _vp, _psz, _vp]),
    "pcx_probe_windows": (_i, [_vp, _vp, _sz, _vp]),
    "pcx_probe_windows_dev": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "pcx_trigger_create": (_i, [C.POINTER(_vp), _i, _i]),
    "pcx_trigger_destroy": (_i, [_vp]),
    "pcx_trigger_set_level": (_i, [_vp, _d]),
    "pcx_trigger_get_level": (_i, [_vp, C.POINTER(_d)]),
    "pcx_trigger_set_slope": (_i, [_vp, _i]),
    "pcx_trigger_get_slope": (_i, [_vp, C.POINTER(_i)]),
    "pcx_trigger_get_geometry": (_i, [_vp, _psz]),
    "pcx_trigger_search": (_i, [_vp, _vp, _sz, _sz, C.POINTER(TriggerHit)]),
    "pcx_trigger_search_dev": (_i, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "pcx_trigger_position": (_d, [C.POINTER(TriggerHit), _d]),
    "pcx_trigger_capture": (_i, [_vp, _sz, C.POINTER(_vp), _psz, _vp, _sz, _sz, C.POINTER(_vp)]),
    "pcx_trigger_capture_dev": (_i, [_vp, _sz, C.POINTER(_vp), _psz, _vp, _sz, _sz, C.POINTER(_vp), _vp]),
    "pcx_framer_create": (_i, [C.POINTER(_vp), _i, _i]),
    "pcx_framer_destroy": (_i, [_vp]),
    "pcx_framer_set_preamble": (_i, [_vp, _vp, _sz, _sz, _i]),
    "pcx_framer_get_preamble": (_i, [_vp, _vp, _sz, _psz, _psz, C.POINTER(_i)]),
    "pcx_framer_set_header_id": (_i, [_vp, C.c_ubyte]),
    "pcx_framer_get_header_id": (_i, [_vp, C.POINTER(C.c_ubyte)]),
    "pcx_framer_set_padding": (_i, [_vp, _sz]),
    "pcx_framer_get_padding": (_i, [_vp, _psz]),
    "pcx_framer_get_geometry": (_i, [_psz, _psz]),
    "pcx_frame_header_bits": (_i, [C.c_uint, C.c_uint, C.POINTER(C.c_uint64)]),
    "pcx_framer_plan": (_i, [_vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz]),
    "pcx_framer_process": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "pcx_framer_process_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "pcx_fsync_create": (_i, [C.POINTER(_vp), _i, _i]),
    "pcx_fsync_destroy": (_i, [_vp]),
    "pcx_fsync_set_output_mode": (_i, [_vp, _i]),
    "pcx_fsync_get_output_mode": (_i, [_vp, C.POINTER(_i)]),
    "pcx_fsync_set_preamble": (_i, [_vp, _vp, _sz]),
    "pcx_fsync_get_preamble": (_i, [_vp, _vp, _sz, _psz]),
    "pcx_fsync_set_header_id": (_i, [_vp, C.c_ubyte]),
    "pcx_fsync_get_header_id": (_i, [_vp, C.POINTER(C.c_ubyte)]),
    "pcx_fsync_set_symbol_width": (_i, [_vp, _sz]),
    "pcx_fsync_get_symbol_width": (_i, [_vp, _psz]),
    "pcx_fsync_set_data_width": (_i, [_vp, _sz]),
    "pcx_fsync_get_data_width": (_i, [_vp, _psz]),
    "pcx_fsync_set_input_threshold": (_i, [_vp, _d]),
    "pcx_fsync_get_input_threshold": (_i, [_vp, C.POINTER(_d)]),
    "pcx_fsync_set_verbose": (_i, [_vp, _i]),
    "pcx_fsync_set_label_id": (_i, [_vp, _i, C.c_char_p]),
    "pcx_fsync_get_label_id": (_i, [_vp, _i, C.c_char_p, _sz, _psz]),
    "pcx_fsync_get_geometry": (_i, [_vp, _psz, _psz, _psz, _psz, _psz, _psz]),
    "pcx_fsync_activate": (_i, [_vp]),
    "pcx_fsync_process": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(FsyncResult)]),
    "pcx_fsync_process_dev": (_i, [_vp, _vp, _sz, _vp, _sz, C.POINTER(FsyncResult), _vp]),
    "pcx_mapper_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "pcx_mapper_destroy": (_i, [_vp]),
    "pcx_mapper_set_map": (_i, [_vp, _vp, _sz]),
    "pcx_mapper_get_map": (_i, [_vp, _vp, _sz, _psz]),
    "pcx_mapper_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_mapper_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_slicer_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "pcx_slicer_destroy": (_i, [_vp]),
    "pcx_slicer_set_map": (_i, [_vp, _vp, _sz]),
    "pcx_slicer_get_map": (_i, [_vp, _vp, _sz, _psz]),
    "pcx_slicer_get_geometry": (_i, [_vp, _psz, _psz, _psz, _psz]),
    "pcx_slicer_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_slicer_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_diffcode_create": (_i, [_i, C.POINTER(_vp)]),
    "pcx_diffcode_destroy": (_i, [_vp]),
    "pcx_diffcode_set_symbols": (_i, [_vp, C.c_uint32]),
    "pcx_diffcode_get_symbols": (_i, [_vp, C.POINTER(C.c_uint32)]),
    "pcx_diffcode_get_plan": (_i, [_vp, C.POINTER(_i)]),
    "pcx_diffcode_get_geometry": (_i, [_psz, _psz]),
    "pcx_diffcode_get_state": (_i, [_vp, C.POINTER(C.c_ubyte)]),
    "pcx_diffcode_reset": (_i, [_vp]),
    "pcx_diffcode_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_diffcode_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_repack_create": (_i, [_i, C.POINTER(_vp)]),
    "pcx_repack_destroy": (_i, [_vp]),
    "pcx_repack_set_modulus": (_i, [_vp, C.c_uint]),
    "pcx_repack_get_modulus": (_i, [_vp, C.POINTER(C.c_uint)]),
    "pcx_repack_set_bit_order": (_i, [_vp, _i]),
    "pcx_repack_get_bit_order": (_i, [_vp, C.POINTER(_i)]),
    "pcx_repack_get_group": (_i, [_vp, _psz, _psz]),
    "pcx_repack_get_geometry": (_i, [_vp, _psz, _psz]),
    "pcx_repack_process": (_i, [_vp, _vp, _vp, _sz]),
    "pcx_repack_process_dev": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "pcx_source_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "pcx_source_destroy": (_i, [_vp]),
    "pcx_source_set_table": (_i, [_vp, _vp, _sz, C.c_uint64]),
    "pcx_source_get_index": (_i, [_vp, C.POINTER(C.c_uint64)]),
    "pcx_source_set_index": (_i, [_vp, C.c_uint64]),
    "pcx_source_get_geometry": (_i, [_vp, _psz, _psz, C.POINTER(_i)]),
    "pcx_source_generate": (_i, [_vp, _vp, _sz]),
    "pcx_source_generate_dev": (_i, [_vp, _vp, _sz, _vp]),
    "pcx_waveform_table": (_i, [_i, _i, _i, _d, _d, _d, _d, _d, _d, _d, _vp, _sz, _psz, C.POINTER(C.c_uint64)]),
    "pcx_noise_create": (_i, [_i, C.c_uint32, C.POINTER(_vp)]),
    "pcx_noise_destroy": (_i, [_vp]),
    "pcx_noise_table": (_i, [_vp, _i, _i, _i, _d, _d, _d, _d, _d, _d, _vp]),
    "pcx_noise_next_offset": (_i, [_vp, _psz]),
    "pcx_rotate": (_i, [_i, _d, _d, _vp, _vp, _sz]),
    "pcx_rotate_dev": (_i, [_i, _d, _d, _vp, _vp, _sz, _vp]),
    "pcx_scale": (_i, [_i, _i, _d, _vp, _vp, _sz]),
    "pcx_scale_dev": (_i, [_i, _i, _d, _vp, _vp, _sz, _vp]),
    "pcx_rotate_q": (_i, [_i, _d, _d, _vp, _vp, _vp, _sz]),
    "pcx_rotate_q_dev": (_i, [_i, _d, _d, _vp, _vp, _vp, _sz, _vp]),
    "pcx_scale_q": (_i, [_i, _i, _d, _vp, _vp, _vp, _sz]),
    "pcx_scale_q_dev": (_i, [_i, _i, _d, _vp, _vp, _vp, _sz, _vp]),
    "pcx_abs": (_i, [_i, _i, _vp, _vp, _sz]),
    "pcx_abs_dev": (_i, [_i, _i, _vp, _vp, _sz, _vp]),
    "pcx_conj": (_i, [_i, _vp, _vp, _sz]),
    "pcx_conj_dev": (_i, [_i, _vp, _vp, _sz, _vp]),
    "pcx_angle": (_i, [_i, _vp, _vp, _sz]),
    "pcx_angle_dev": (_i, [_i, _vp, _vp, _sz, _vp]),
    "pcx_arith": (_i, [_i, _i, _i, _vp, _vp, _vp, _sz]),
    "pcx_arith_dev": (_i, [_i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_compare": (_i, [_i, _i, _vp, _vp, _vp, _sz]),
    "pcx_compare_dev": (_i, [_i, _i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_compare_const": (_i, [_i, _i, _vp, _vp, _vp, _sz]),
    "pcx_compare_const_dev": (_i, [_i, _i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_bitwise": (_i, [_i, _i, C.POINTER(_vp), _sz, _vp, _sz]),
    "pcx_bitwise_dev": (_i, [_i, _i, C.POINTER(_vp), _sz, _vp, _sz, _vp]),
    "pcx_bitwise_const": (_i, [_i, _i, _vp, _vp, _vp, _sz]),
    "pcx_bitwise_const_dev": (_i, [_i, _i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_bitshift": (_i, [_i, _i, _vp, _sz, _vp, _sz]),
    "pcx_bitshift_dev": (_i, [_i, _i, _vp, _sz, _vp, _sz, _vp]),
    "pcx_byteswap": (_i, [_i, _vp, _vp, _sz]),
    "pcx_byteswap_dev": (_i, [_i, _vp, _vp, _sz, _vp]),
    "pcx_arith_const": (_i, [_i, _i, _i, _vp, _vp, _vp, _sz]),
    "pcx_arith_const_dev": (_i, [_i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_mathfn": (_i, [_i, _i, _vp, _vp, _sz]),
    "pcx_mathfn_dev": (_i, [_i, _i, _vp, _vp, _sz, _vp]),
    "pcx_mathfn_param": (_i, [_i, _i, _vp, _vp, _vp, _sz]),
    "pcx_mathfn_param_dev": (_i, [_i, _i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_specfn": (_i, [_i, _i, _vp, _vp, _sz]),
    "pcx_specfn_dev": (_i, [_i, _i, _vp, _vp, _sz, _vp]),
    "pcx_beta": (_i, [_i, _vp, _vp, _vp, _sz]),
    "pcx_beta_dev": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_modf": (_i, [_i, _vp, _vp, _vp, _sz]),
    "pcx_modf_dev": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_split_complex": (_i, [_i, _vp, _vp, _vp, _sz]),
    "pcx_split_complex_dev": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_combine_complex": (_i, [_i, _vp, _vp, _vp, _sz]),
    "pcx_combine_complex_dev": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
    "pcx_fmchain_create": (_i, [C.POINTER(_vp)]),
    "pcx_fmchain_destroy": (_i, [_vp]),
    "pcx_fmchain_set_phase": (_i, [_vp, _d]),
    "pcx_fmchain_set_taps": (_i, [_vp, _vp, _sz, _i]),
    "pcx_fmchain_reset": (_i, [_vp]),
    "pcx_fmchain_set_algo": (_i, [_vp, _i]),
    "pcx_fmchain_last_algo": (_i, [_vp]),
    "pcx_fmchain_set_slots": (_i, [_vp, C.c_uint]),
    "pcx_fmchain_process": (_i, [_vp, _vp, _sz, _vp, _sz, _psz, _psz]),
    "pcx_fmchain_process_dev": (_i, [_vp, _vp, _sz, _vp, _sz, _psz, _psz, _vp]),
    "pcx_fmchain_process_dev_gated": (_i, [_vp, _vp, _sz, _vp, _sz, _psz, _psz, _vp, C.c_uint, _vp, C.POINTER(C.c_int)]),
    "pcx_shard_create": (_i, [_i, C.POINTER(C.c_int), _i, C.POINTER(_vp)]),
    "pcx_shard_destroy": (_i, [_vp]),
    "pcx_shard_set_taps": (_i, [_vp, C.POINTER(C.c_double), _sz, _i]),
    "pcx_shard_set_gated": (_i, [_vp, _i]),
    "pcx_shard_set_submit_threads": (_i, [_vp, _i]),
    "pcx_shard_set_algo": (_i, [_vp, _i]),
    "pcx_shard_set_chain": (_i, [_vp, _i, _d]),
    "pcx_shard_configure": (_i, [_vp, _sz]),
    "pcx_shard_info": (_i, [_vp, C.POINTER(C.c_int), _psz, _psz, C.POINTER(C.c_int)]),
    "pcx_shard_buffers": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int)]),
    "pcx_shard_scatter": (_i, [_vp, _vp, _sz]),
    "pcx_shard_step": (_i, [_vp]),
    "pcx_shard_post_exchange": (_i, [_vp]),
    "pcx_shard_compute": (_i, [_vp]),
    "pcx_shard_gather": (_i, [_vp, _vp, _sz]),
    "pcx_shard_sync": (_i, [_vp]),
}

_lib = None
_hip_runtime = None


def _preload_hip_runtime():
    """One HIP runtime per process.

    libpcx_hip.so needs `libamdhip64.so.7`.  PyTorch-ROCm wheels bundle their own copy
    (same SONAME) and load it by path; a process that ends up with both the system copy and
    torch's copy has two runtimes fighting over the device (the second one reports "no
    ROCm-capable device").  Whoever loads first decides, so when torch is installed we map
    torch's copy first -- by SONAME match libpcx_hip.so then binds to it, and a later
    `import torch` reuses the same mapping.  Without torch the RUNPATH (/opt/rocm/lib) copy
    is used.  PCX_HIP_RUNTIME=<path> overrides.
    """
    global _hip_runtime
    if _hip_runtime is not None:
        return
    path = os.environ.get("PCX_HIP_RUNTIME")
    if not path:
        try:
            import importlib.util
            spec = importlib.util.find_spec("torch")
            if spec is not None and spec.submodule_search_locations:
                cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
                if os.path.exists(cand):
                    path = cand
        except (ImportError, ValueError):
            path = None
    if path:
        _hip_runtime = C.CDLL(path, mode=C.RTLD_GLOBAL)
    else:
        _hip_runtime = False


def load():
    """Load libpcx_hip.so (raises if it is not built -- no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    # tools/ only: PCX_HIP_LIBRARY points the loader at the diagnostic build (make -C pothoscomms_amd/csrc diag),
    # the one library that reads A/B switches from the environment and holds the timing-only kernel variants
    override = os.environ.get("PCX_HIP_LIBRARY")
    if override:
        if not os.path.exists(override):
            raise ImportError("PCX_HIP_LIBRARY=%s does not exist" % override)
        path = override
    if not os.path.exists(path):
        raise ImportError(
            "%s is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C pothoscomms_amd/csrc).  pothoscomms_amd has no CPU fallback." % LIB_PATH)
    _preload_hip_runtime()
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load().pcx_last_error().decode("utf-8", "replace")


def check(status):
    if status == OK:
        return
    msg = last_error()
    if status == ERR_ARG:
        raise InvalidArgument(status, msg)
    if status == ERR_UNSUPPORTED:
        raise Unsupported(status, msg)
    raise PcxError(status, msg)
