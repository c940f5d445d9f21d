"""Model of /comms/threshold (utility/Threshold.cpp:130-144) in two formulations.

An element x is compared with the two levels in the element type itself: a = x > activation, d = x < deactivation (a NaN on either
side compares false).  With the state s before the element, the state after it is a if s is inactive, not d if it is active.

  states_loop   the reference's loop, element by element
  states_scan   every element is an affine map s -> m s + b over GF(2), with b = a (the image of inactive) and m = a xor not d
                (1: keep or toggle, 0: set or clear).  Composed in closed form: the state after element i is the constant b[j] of
                the last element j <= i with m = 0 (the entry state when there is none), toggled once per element with m = b = 1
                behind j.  A few passes of numpy over the stream: fast enough for 64 Mi elements.

Both return the state AFTER every element as uint8; transitions() turns that into the ascending indices at which the state
changed.  Transition j is an activation exactly when (entry + j) is even."""
import numpy as np

TYPES = ["float64", "float32", "int64", "int32", "int16", "int8"]


def level(dtype, v):
    """v as one element of dtype (numpy's conversion, as device.Threshold converts)"""
    return np.array([v], dtype=np.dtype(dtype))[0]


def flags(x, act, deact):
    x = np.ascontiguousarray(x)
    assert x.ndim == 1 and x.dtype.name in TYPES, x.dtype
    with np.errstate(invalid="ignore"):
        return x > level(x.dtype, act), x < level(x.dtype, deact)


def states_loop(x, act, deact, entry=0):
    a, d = flags(x, act, deact)
    out = np.zeros(a.size, np.uint8)
    s = bool(entry)
    for i, (ai, di) in enumerate(zip(a.tolist(), d.tolist())):
        if not s and ai:
            s = True
        elif s and di:
            s = False
        out[i] = s
    return out


def states_scan(x, act, deact, entry=0):
    a, d = flags(x, act, deact)
    n = a.size
    if n == 0:
        return np.zeros(0, np.uint8)
    b = a.view(np.uint8)
    m = b ^ (~d).view(np.uint8)
    par = np.cumsum(m & b, dtype=np.uint8) & 1              # toggles up to and including i, mod 2 (a wrapping sum keeps the parity)
    it = np.int32 if n < (1 << 31) else np.int64
    j = np.where(m == 0, np.arange(n, dtype=it), it(-1))
    np.maximum.accumulate(j, out=j)                         # the last set / clear at or in front of i
    has = j >= 0
    j[~has] = 0
    base = np.where(has, b[j], np.uint8(bool(entry)))
    pj = np.where(has, par[j], np.uint8(0))
    return (base ^ par ^ pj).astype(np.uint8)


def transitions(states, entry=0):
    """ascending indices (uint64) of the elements at which the state changed"""
    s = np.asarray(states, np.uint8)
    prev = np.empty_like(s)
    if s.size:
        prev[0] = bool(entry)
        prev[1:] = s[:-1]
    return np.nonzero(s != prev)[0].astype(np.uint64)


def run(x, act, deact, entry=0, states=states_scan):
    """(transition indices, count, entry state, state behind the stream, states)"""
    s = states(x, act, deact, entry)
    idx = transitions(s, entry)
    return idx, int(idx.size), int(bool(entry)), int(s[-1]) if s.size else int(bool(entry)), s


def kinds(n_transitions, entry):
    """1 for an activation, 0 for a deactivation, by the alternation rule"""
    return ((np.arange(n_transitions) + int(bool(entry))) % 2 == 0).astype(np.uint8)


def run_cuts(work, x, cuts):
    """Feeds x to work(buf) -> indices in calls of `cuts` elements (the last cut may be None: the rest) and returns the indices
    rebased by the elements consumed so far."""
    out, pos = [], 0
    for c in cuts:
        c = x.size - pos if c is None else c
        idx = np.asarray(work(x[pos:pos + c]), np.uint64)
        out.append(idx + np.uint64(pos))
        pos += c
    assert pos == x.size, (pos, x.size)
    return np.concatenate(out) if out else np.zeros(0, np.uint64)
