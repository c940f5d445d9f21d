"""Model of the two source blocks for the tests (numpy, no device): the cyclic walk of a table from a carried 64-bit index
(waveform/WaveformSource.cpp:98-108, waveform/NoiseSource.cpp:109-117) and the case lists of tests/golden/source.npz."""
import hashlib

import numpy as np

M64 = (1 << 64) - 1
SCALARS = ("float64", "float32", "int64", "int32", "int16", "int8")
TYPES = tuple(s for s in SCALARS) + tuple("complex_" + s for s in SCALARS)
WAVES = ("CONST", "SINE", "RAMP", "SQUARE")
NOISE_WAVES = ("UNIFORM", "NORMAL", "LAPLACE", "POISSON")
FURTHER_TYPES = ("complex_float32", "complex_int16", "float64")
NOISE_TYPES = ("complex_float64", "float32", "complex_int16")
CALLS = (257, 300, 43)
NOISE_SEED = 20261018
NOISE_MEAN, NOISE_B = 0.5, 0.25
NOISE_CALLS = (100,) * 5


def is_complex(dtype):
    return dtype.startswith("complex_")


def is_integer(dtype):
    return "int" in dtype


def np_scalar(dtype):
    return np.dtype(dtype[8:] if is_complex(dtype) else dtype)


def elem_bytes(dtype):
    return np_scalar(dtype).itemsize * (2 if is_complex(dtype) else 1)


def shape(dtype, n):
    return (n, 2) if is_complex(dtype) else (n,)


def ampl_offset(dtype):
    """the matrix's amplitude and offset: 100 and (25, -50) for the integer types (fits int8), 1 and (0.25, -0.5) otherwise"""
    k = 100.0 if is_integer(dtype) else 1.0
    return (k, 0.0), (0.25 * k, -0.5 * k)


def walk(table, index, step, n):
    """(out, index afterwards): out[i] = table[(index + i * step) & (size - 1)], the arithmetic modulo 2^64"""
    size = table.shape[0]
    assert size & (size - 1) == 0
    step &= M64
    # the low bits of the walk are all that reach the mask, so the 64-bit wrap needs no wide arithmetic
    pos = (np.uint64(index & (size - 1)) + np.arange(n, dtype=np.uint64) * np.uint64(step & (size - 1))) & np.uint64(size - 1)
    return table[pos.astype(np.int64)], (index + n * step) & M64


def period(size, step):
    s = step & (size - 1)
    return 1 if s == 0 else size // min(s & -s, size)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def waveform_cases():
    """[(name, dtype, wave, [op, ...])]: ops are ("freq", f), ("res", r), ("work", n) applied after rate 1 and the type's amplitude and offset;
    the block is activated in front of the first of them"""
    cases = []
    three = [("work", n) for n in CALLS]
    for dt in TYPES:
        for w in WAVES:
            cases.append(("matrix/%s/%s" % (dt, w), dt, w, [("freq", 0.1)] + three))
    for dt in FURTHER_TYPES:
        cases.append(("neg/%s" % dt, dt, "SINE", [("freq", -0.25)] + three))
        cases.append(("zero/%s" % dt, dt, "SINE", [("freq", 0.0)] + three))
        cases.append(("slow/%s" % dt, dt, "SINE", [("freq", 1e-4), ("work", 600)]))
        cases.append(("slowest/%s" % dt, dt, "SINE", [("freq", 1e-6), ("work", 600)]))
        cases.append(("res/%s" % dt, dt, "SINE", [("res", 1e-3), ("freq", 0.1)] + three))
        cases.append(("retune/%s" % dt, dt, "SINE", [("freq", 0.1), ("work", 300), ("freq", 1e-4), ("work", 300)]))
    return cases


def noise_cases():
    return [("noise/%s/%s" % (dt, w), dt, w) for dt in NOISE_TYPES for w in NOISE_WAVES]
