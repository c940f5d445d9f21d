"""Model of /comms/frame_sync: the yardstick of tests/test_framesync_cpu.py and tests/test_framesync_gpu.py.

`Model(settings, ft)` states digital/FrameSync.cpp's work() on the ABSOLUTE stream under a call schedule: a call is `work(pos, n_in,
out_cap)` on the elements [pos, pos + n_in) of the stream given at construction; elements in front of the stream read as zero (the
port's history after activate()).  `ft` is the floating type everything is computed in, in the reference's order of operations (sums
run in stream order, the rotation's angle is a running sum): numpy.float64 is the truth for complex_float32 streams, numpy.longdouble
the truth for complex_float64 streams, and numpy.float32 / numpy.float64 restate the reference's two instantiations.  Only the payload's
phase is in closed form (phase0 + k inc), as on the device.

The model records the MARGIN of every comparison that steers control flow or an integer, at the offsets and frames a schedule visits:
  env   the four envelope thresholds and the two ratio bounds, relative: |value - bound| / bound
  int   the distance of |L| from the nearest integer wherever |L| >= corrMagThresh - 1
  bit   every comparison of bit.real() in the first-bit search and the 58 bit decisions, absolute, the symbol scaled to modulus 1
`condition(margins)` is the cap every fixture and generated stream must meet before anything is compared (ISSUE: 0.05, 0.1, 0.01).

`frame`, `build` and `channel` make test streams from framer_model's frame layout with the two shapings that take the decisions off
their edges; `tuned` chooses the noise seed and the dip under which a stream meets the condition; `CASES` is the list the CPU suite, the
GPU suite and the recorded reference share."""
import collections
import functools
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import framer_model

HEADER_BITS = framer_model.HEADER_BITS
MODES = ("RAW", "PHASE", "TIMING", "DEBUG")
CAP_ENV, CAP_INT, CAP_BIT = 0.05, 0.1, 0.01
LABEL_KINDS = ("phase_offset", "frame_start", "frame_end")
# the recorded reference (tests/golden/make_framesync_golden.py); None: streams are chosen afresh and the restatement stands in
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "framesync.npz")

Settings = collections.namedtuple("Settings", "sw dw preamble header_id mode thresh start_id end_id phase_id")
Call = collections.namedtuple("Call", "consumed produced reserve labels out state")


def settings(sw=20, dw=4, preamble=(1,), header_id=0x55, mode="RAW", thresh=0.01, start_id="frameStart", end_id="", phase_id=""):
    return Settings(sw, dw, np.asarray(preamble, np.complex128), header_id, mode, thresh, start_id, end_id, phase_id)


def derived(s):
    """(W, F, corrMagThresh, corrDurThresh)"""
    W = s.sw * s.dw * len(s.preamble)
    return W, W + HEADER_BITS * s.dw, int(W * 0.7), int(W * 0.5)


def ctype(ft):
    return {np.float32: np.complex64, np.float64: np.complex128, np.longdouble: np.clongdouble}[ft]


def seqsum(a):
    """the sum along the last axis in index order, in the array's own type"""
    if a.shape[-1] == 0:
        return np.zeros(a.shape[:-1], a.dtype)
    return np.cumsum(a, axis=-1)[..., -1]


def polar(r, phi):
    return (r * np.cos(phi)) + 1j * (r * np.sin(phi))


class Model:
    def __init__(self, s, ft, stream):
        self.s, self.ft, self.ct = s, ft, ctype(ft)
        self.W, self.F, self.mag, self.dur = derived(s)
        self.pad = self.dur + 2
        # the threshold and the preamble in the precision of the STREAM the model stands for
        self.thr = ft(np.float32(s.thresh)) if stream.dtype == np.complex64 else ft(s.thresh)
        self.pre = s.preamble.astype(stream.dtype).astype(self.ct)
        self.x = np.concatenate([np.zeros(self.pad, self.ct), np.asarray(stream).astype(self.ct)])
        self.margins = dict(env=[], int=[], bit=[])
        self.peaks_seen = []            # (absolute offset, |L|) of every visited offset with an open gate
        self._metric()
        self.activate()

    def activate(self):
        self.remaining, self.max_peak, self.cnt, self.reserve = 0, 0, 0, 0
        self.phase = self.phase_inc = self.ft(0)
        self.scale = self.dfc = self.poff = self.ft(0)

    def at(self, i):
        """element i of the stream (zero in front of it)"""
        return self.x[i + self.pad]

    # ---- the three estimates at every offset of the stream at once
    def _metric(self):
        s, ft, W = self.s, self.ft, self.W
        x = self.x[self.pad:]
        M = len(x) - W + 1
        self.M = max(M, 0)
        if M <= 0:
            return
        a = np.abs(x).astype(ft)
        win, awin = sliding_window_view(x, W), sliding_window_view(a, W)
        thr, half, dw = self.thr, s.sw * s.dw // 2, s.dw
        rel = lambda v, b: np.abs(v - b) / b
        env = np.full(M, np.inf)
        g = awin[:, dw] >= thr
        env = np.minimum(env, rel(awin[:, dw], thr))
        alive = g.copy()
        v = awin[:, W - dw]
        env = np.where(alive, np.minimum(env, rel(v, thr)), env)
        alive &= v >= thr
        sum0 = seqsum(awin[:, dw:half]) / ft(half - dw)
        env = np.where(alive, np.minimum(env, rel(sum0, thr)), env)
        alive &= sum0 >= thr
        sum0 = sum0 / ft(abs(self.pre[0]))
        sum1 = seqsum(awin[:, W - half:W - dw]) / ft(half - dw)
        env = np.where(alive, np.minimum(env, rel(sum1, thr)), env)
        alive &= sum1 >= thr
        sum1 = sum1 / ft(abs(self.pre[-1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = sum0 / sum1
            env = np.where(alive, np.minimum(env, np.minimum(rel(ratio, ft(2)), rel(ratio, ft(0.5)))), env)
            alive &= ~((ratio > 2) | (ratio < 0.5))
            scale = np.where(alive, ft(2) / (sum0 + sum1), ft(0)).astype(ft)
        self.env_margin = env
        self.scale_at = scale
        rows = np.flatnonzero(alive)
        self.dfc_at, self.poff_at, self.L_at = np.zeros(M, ft), np.zeros(M, ft), np.zeros(M, ft)
        if not rows.size:
            return
        width = s.sw * s.dw
        base, delta = width * (len(self.pre) - 1), width // 2
        end = width - delta - dw
        w = win[rows]
        if end > dw:
            K = seqsum(w[:, base + dw:base + end] * np.conj(w[:, base + dw + delta:base + end + delta]))
            dfc = (np.arctan2(K.imag, K.real) / ft(delta)).astype(ft)
        else:
            dfc = np.zeros(rows.size, ft)
        # freqCorr: 0, then the running sum of deltaFc, in ft
        fc = np.zeros((rows.size, W), ft)
        if W > 1:
            fc[:, 1:] = np.cumsum(np.repeat(dfc[:, None], W - 1, axis=1), axis=1)
        sym = np.conj(np.repeat(self.pre, width))
        L = seqsum(((sym[None, :] * w) * polar(scale[rows][:, None], fc)).astype(self.ct))
        self.dfc_at[rows] = dfc
        self.poff_at[rows] = -np.arctan2(L.imag, L.real)
        self.L_at[rows] = np.abs(L)

    # ---- processHeaderBits
    def _header(self, fo, scale, dfc, poff):
        s, ft, W, F = self.s, self.ft, self.W, self.F
        sym = np.conj(self.pre[-1])
        unit = float(abs(sym))
        first, peak = W + s.dw // 2, ft(0)
        for i in range(W - (s.dw * s.sw // 2), F):
            bit = (self.at(fo + i) * polar(scale, poff + dfc * ft(i))) * sym
            self.margins["bit"].append(abs(float(bit.real) - float(peak)) / unit)
            if bit.real > peak:
                if peak == 0:
                    continue
                break
            first, peak = i, ft(bit.real)
        if peak == 0:
            return first, None
        bits, fc = [], poff + dfc * ft(first)
        for k in range(HEADER_BITS):
            bit = (self.at(fo + first + k * s.dw) * polar(scale, fc)) * sym
            self.margins["bit"].append(abs(float(bit.real)) / unit)
            bits.append(1 if bit.real > 0 else 0)
            fc = fc + dfc * ft(s.dw)
        return first, bits

    def state(self):
        return dict(remaining=self.remaining, phase=self.phase, phase_inc=self.phase_inc, scale=self.scale, delta_fc=self.dfc, phase_off=self.poff,
                    max_peak=self.max_peak, count_since_max=self.cnt)

    # ---- one work()
    def work(self, pos, n_in, out_cap):
        s, ft = self.s, self.ft
        empty = np.zeros(0, self.ct)
        if self.remaining:
            if s.mode == "TIMING":
                N = min(min(self.remaining, n_in) // s.dw, out_cap)
                if N == 0:
                    self.reserve = s.dw
                k = np.arange(N)
                out = self.x[self.pad + pos + k * s.dw] * polar(self.scale, self.phase + k.astype(ft) * (self.phase_inc * ft(s.dw)))
                self.phase = self.phase + ft(N) * (self.phase_inc * ft(s.dw))
                consumed = N * s.dw
            else:
                N = min(self.remaining, n_in, out_cap)
                seg = self.x[self.pad + pos:self.pad + pos + N]
                if s.mode == "RAW":
                    out = seg * self.scale
                else:
                    out = seg * polar(self.scale, self.phase + np.arange(N).astype(ft) * self.phase_inc)
                    self.phase = self.phase + ft(N) * self.phase_inc
                consumed = N
            self.remaining -= consumed
            return Call(consumed, N, self.reserve, [], out.astype(self.ct), self.state())
        if n_in < self.F:
            self.reserve = self.F
            return Call(0, 0, self.reserve, [], empty, self.state())
        N = n_in - self.F + 1
        for i in range(N):
            o = pos + i
            self.margins["env"].append(float(self.env_margin[o]))
            peak = 0
            if self.scale_at[o] != 0:
                L = self.L_at[o]
                self.peaks_seen.append((o, float(L)))
                if L >= self.mag - 1:
                    self.margins["int"].append(abs(float(L) - round(float(L))))
                peak = int(L)
            if peak > self.max_peak and peak > self.mag:
                self.max_peak, self.cnt = peak, 0
                self.dfc, self.poff, self.scale = self.dfc_at[o], self.poff_at[o], self.scale_at[o]
            self.cnt += 1
            if self.max_peak < self.mag or self.cnt < self.dur:
                continue
            self.max_peak = 0
            fo = o - self.cnt
            first, bits = self._header(fo, self.scale, self.dfc, self.poff)
            if bits is None:
                continue
            hid, length, chk, bad = framer_model.header_decode(bits)
            if bad or chk != framer_model.header_checksum(hid, length) or hid != s.header_id or length == 0:
                continue
            lw = 1 if s.mode == "TIMING" else s.dw
            payload = (fo - pos) + first + HEADER_BITS * s.dw + lw // 2
            l0, l1 = 0, (length - 1) * lw
            self.remaining = length * s.dw
            self.phase_inc = self.dfc
            self.phase = self.poff + self.phase_inc * ft(self.F)
            if s.mode == "DEBUG":
                backup = min(payload, self.F)
                l0, l1 = l0 + backup, l1 + backup
                self.phase = self.phase - self.phase_inc * ft(backup)
                self.remaining += backup
                payload -= backup
            labels = []
            if s.phase_id:
                labels.append(("phase_offset", l0, lw, self.phase))
            if s.start_id:
                labels.append(("frame_start", l0, lw, length))
            if s.end_id:
                labels.append(("frame_end", l1, lw, length))
            self.reserve = 0
            return Call(payload, 0, self.reserve, labels, empty, self.state())
        return Call(N, 0, self.reserve, [], empty, self.state())

    def run(self, feed, out_cap=None, max_calls=10000):
        """the calls of a feed schedule: feed[k] is how many elements past the consumed ones call k sees (the last entry repeats); the
        loop ends when a call with the whole rest of the stream in view consumes and produces nothing.  -> [Call]"""
        pos, total, calls = 0, len(self.x) - self.pad, []
        for k in range(max_calls):
            n_in = min(feed[min(k, len(feed) - 1)], total - pos)
            c = self.work(pos, n_in, n_in if out_cap is None else out_cap)
            calls.append(c)
            pos += c.consumed
            if c.consumed == 0 and c.produced == 0 and n_in == total - pos:
                break
        return calls


def condition(margins):
    """the margin condition of the parity contract -> (ok, the three minima)"""
    m = tuple(min(margins[k]) if margins[k] else np.inf for k in ("env", "int", "bit"))
    return (m[0] >= CAP_ENV and m[1] >= CAP_INT and m[2] >= CAP_BIT), m


# ---- streams
def frame(s, length, payload, header_id=None, flip=(), dip=0.5, shape=0.04):
    """one frame as float64 samples of amplitude 1: the preamble with every symbol held sw * dw samples, the 58 header symbols and the
    payload symbols held dw samples each.  dip: the middle preamble symbol is lowered by this much in all, spread over samples that
    neither the envelope nor the frequency estimate reads (the whole symbol where the preamble has three or more, else its transition
    padding), which moves the peak |L| from an integer to the middle between two.  shape: a held data symbol rises by this much per
    sample up to its middle sample dw // 2 and falls behind it, which makes the first-bit search's minimum unique.  flip: header
    symbols to negate.  length: the header's length field (the payload may be shorter or longer than it says)."""
    width, P = s.sw * s.dw, len(s.preamble)
    pre = np.repeat(s.preamble.astype(np.complex128), width)
    if dip:
        mid = P // 2
        where = np.arange(width) if P >= 3 else np.concatenate([np.arange(s.dw), np.arange(width - s.dw + 1, width)])
        pre[mid * width + where] *= 1.0 - dip / len(where) / abs(s.preamble[mid])
    bits = framer_model.header_bits(s.header_id if header_id is None else header_id, length & 0xFFFF)
    sym = s.preamble[-1]
    hdr = np.array([sym if b else -sym for b in bits], np.complex128)
    for k in flip:
        hdr[k] = -hdr[k]
    k = np.arange(s.dw)
    bump = 1.0 + shape * np.where(k <= s.dw // 2, k, 2 * (s.dw // 2) - k)
    held = lambda v: (np.repeat(v, s.dw).reshape(-1, s.dw) * bump[None, :]).reshape(-1)
    return np.concatenate([pre, held(hdr), held(np.asarray(payload, np.complex128))])


def qpsk(rng, n):
    return np.exp(1j * (np.pi / 4 + np.pi / 2 * rng.integers(0, 4, n)))


def channel(x, rng, ampl=1.0, phase=0.0, freq=0.0, noise=1e-3, dtype=np.complex64):
    """amplitude, phase and frequency offset, and noise relative to the amplitude, as a stream of `dtype`"""
    k = np.arange(len(x))
    w = (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * (noise * ampl / np.sqrt(2))
    return (ampl * x * np.exp(1j * (phase + freq * k)) + w).astype(dtype)


def decisions(calls):
    """what must be equal exactly: per call consumed, produced, reserve, the labels' kinds, indices, widths and lengths, the tracker"""
    return [(c.consumed, c.produced, c.reserve, [(l[0], l[1], l[2], l[3] if l[0] != "phase_offset" else None) for l in c.labels],
             c.state["remaining"], c.state["count_since_max"]) for c in calls]


def tuned(make, feed, out_cap=None, seeds=range(48), dips=(0.5, 0.4, 0.6)):
    """make(seed, dip) -> (settings, stream): the first choice of noise seed and dip under which the stream meets the margin condition
    on this schedule and the restatements in the stream's own precision and in the truth's agree on every decision.  A case is never
    dropped: with no such choice this raises.  -> (settings, stream, truth model, its calls, the restatement's calls, margins)"""
    for dip in dips:
        for seed in seeds:
            s, x = make(seed, dip)
            own, truth = (np.float32, np.float64) if x.dtype == np.complex64 else (np.float64, np.longdouble)
            mt, mo = Model(s, truth, x), Model(s, own, x)
            ct, co = mt.run(feed, out_cap), mo.run(feed, out_cap)
            ok_t, m_t = condition(mt.margins)
            ok_o, m_o = condition(mo.margins)
            if ok_t and ok_o and decisions(ct) == decisions(co):
                return s, x, mt, ct, co, tuple(min(a, b) for a, b in zip(m_t, m_o))
    raise AssertionError("no seed and dip meet the margin condition")


def build(s, items, rng, dip):
    """a stream of amplitude 1 from ("gap", n) | ("carrier", n) | ("frame", length, {frame's keywords}) items; -> (samples, where each
    frame begins, the payload symbols of each frame)"""
    parts, starts, payloads, n = [], [], [], 0
    for it in items:
        if it[0] == "gap":
            part = np.zeros(it[1], np.complex128)
        elif it[0] == "carrier":
            part = np.ones(it[1], np.complex128)
        else:
            kw = dict(it[2]) if len(it) > 2 else {}
            pay = qpsk(rng, kw.pop("symbols", it[1]))
            part = frame(s, it[1], pay, dip=dip, **kw)
            starts.append(n)
            payloads.append(pay)
        parts.append(part)
        n += len(part)
    return np.concatenate(parts), starts, payloads


Case = collections.namedtuple("Case", "name dtype settings items feed out_cap chan")
PRE = {1: (1,), 2: (1, -1), 3: (1, 1, -1), 5: (1, 1, -1, 1, 0.6 + 0.8j),
       105: tuple((2 * np.random.default_rng(105).integers(0, 2, 105) - 1).tolist())}


def _case(name, dtype, sw, dw, P, items, mode="RAW", feed=(1 << 30,), out_cap=None, ids=("frameStart", "e", "p"), freq=None, ampl=0.8, noise=1.5e-3,
          header_id=0x55):
    st = settings(sw=sw, dw=dw, preamble=PRE[P], mode=mode, header_id=header_id, start_id=ids[0], end_id=ids[1], phase_id=ids[2])
    if freq is None:
        freq = 0.0 if sw < 5 else 0.02          # (symbol widths 3 and 4 have no frequency estimate: deltaFc = 0)
    return Case(name, dtype, st, tuple(items), tuple(feed), out_cap, dict(ampl=ampl, phase=0.7, freq=freq, noise=noise))


def _cases():
    out = []
    c32, c64 = "complex_float32", "complex_float64"
    shapes = [(3, 2, 1), (4, 2, 2), (5, 3, 2), (6, 2, 5), (8, 4, 3)]
    k = 0
    for mode in MODES:
        for length in (1, 2, 19):
            sw, dw, P = shapes[k % len(shapes)]
            dt = (c32, c64)[k % 2]
            F = sw * dw * P + HEADER_BITS * dw
            out.append(_case("%s_len%d_%d_%d_p%d" % (mode.lower(), length, sw, dw, P), dt, sw, dw, P, [("gap", 37), ("frame", length), ("gap", F + 50)], mode=mode,
                             freq=(0.0 if sw < 5 else (0.02, -0.03, 0.01)[k % 3])))
            k += 1
    F = 6 * 2 * 5 + HEADER_BITS * 2
    out.append(_case("back_to_back", c32, 6, 2, 5, [("gap", 20), ("frame", 7), ("frame", 5), ("gap", F + 30)], mode="PHASE"))
    out.append(_case("three_apart", c64, 6, 2, 5, [("gap", 20), ("frame", 7), ("gap", 3), ("frame", 5), ("gap", F + 30)], mode="TIMING"))
    out.append(_case("peak_at_0", c32, 5, 3, 2, [("frame", 6), ("gap", 300)], mode="PHASE"))
    out.append(_case("peak_at_1", c64, 5, 3, 2, [("gap", 1), ("frame", 6), ("gap", 300)], mode="DEBUG"))
    # 5/3, two symbols: W 30, F 204, corrDurThresh 15; a frame at 40 peaks at offset 40 and is declared at 54
    F = 204
    out.append(_case("declared_next_call", c32, 5, 3, 2, [("gap", 40), ("frame", 9), ("gap", 300)], mode="PHASE", feed=(F + 45, 1 << 30)))
    out.append(_case("cut_in_sync_word", c64, 5, 3, 2, [("gap", 40), ("frame", 9), ("gap", 300)], mode="RAW", feed=(F + 10, 60, 1 << 30)))
    out.append(_case("cut_in_header", c32, 5, 3, 2, [("gap", 40), ("frame", 9), ("gap", 300)], mode="TIMING", feed=(F + 20, 100, 1 << 30)))
    out.append(_case("cut_in_payload", c64, 5, 3, 2, [("gap", 40), ("frame", 9), ("gap", 300)], mode="PHASE", feed=(F + 60, 11, 4, 1, 1 << 30)))
    out.append(_case("timing_cap_1", c32, 8, 4, 3, [("gap", 10), ("frame", 5), ("gap", 400)], mode="TIMING", out_cap=1))
    out.append(_case("timing_cap_dw_less_1", c64, 8, 4, 3, [("gap", 10), ("frame", 5), ("gap", 400)], mode="TIMING", out_cap=3, feed=(1 << 30, 3, 1 << 30)))
    # a header that fails, of each kind, and a good frame behind it: as near as a frame can follow (the rejected frame has no payload, the
    # next sync word begins where its header ends, the scan going on with the count not reset) and far behind it
    bad = dict(wrong_id=dict(header_id=0xD5), length_0=None, one_flip=dict(flip=(13,)), two_flips=dict(flip=(19, 22)))
    for k, (name, kw) in enumerate(bad.items()):
        first = lambda n: ("frame", 0, dict(symbols=n)) if kw is None else ("frame", 3, dict(kw, symbols=n))
        dt = (c32, c64)[k % 2]
        out.append(_case(name + "_then_near", dt, 6, 2, 5, [("gap", 25), first(3 if name == "one_flip" else 0), ("frame", 4), ("gap", 250)], mode="PHASE"))
        out.append(_case(name + "_then_far", dt, 8, 4, 3, [("gap", 25), first(0), ("gap", 700), ("frame", 4), ("gap", 400)], mode="RAW"))
    out.append(_case("silence", c32, 6, 2, 5, [("gap", 700)]))
    out.append(_case("carrier", c64, 4, 2, 3, [("gap", 30), ("carrier", 600), ("gap", 200)]))
    out.append(_case("below_threshold", c32, 6, 2, 5, [("gap", 30), ("frame", 5), ("gap", 300)], ampl=0.001, noise=0.02))
    # sync words longer than one and than two chunks of the search kernel's staging (768 samples): W = 1050 and W = 1575.  The preamble
    # is 105 pseudo-random signs: with some fifty sign changes |L| falls by about a hundred per offset, so only a handful of offsets
    # around the peak lie above corrMagThresh - 1 and have to keep their distance from an integer (under the 13-symbol Barker code at
    # the default widths some thirty do, at distances the noise decides: a chance of about 0.8^30 per stream, and none of 144 tried met it)
    for dt in (c32, c64):
        F = 5 * 2 * 105 + HEADER_BITS * 2
        out.append(_case("two_chunks_" + dt[8:], dt, 5, 2, 105, [("gap", 53), ("frame", 11), ("gap", F + 40)], mode="PHASE" if dt == c32 else "TIMING", freq=0.004,
                         noise=5e-4))
        F = 5 * 3 * 105 + HEADER_BITS * 3
        out.append(_case("three_chunks_" + dt[8:], dt, 5, 3, 105, [("gap", 29), ("frame", 7), ("gap", F + 40)], mode="DEBUG" if dt == c32 else "PHASE", freq=-0.003,
                         noise=5e-4))
    return out


CASES = _cases()


def prepare(case, seeds=range(48)):
    """a case without a recording: the stream is chosen here (`tuned`) and the restatement in the stream's own precision stands in for
    the reference.  -> (case, settings, stream, truth model, its calls, the stand-in's calls, margins, frame starts, payload symbols)"""
    dt = np.complex64 if case.dtype == "complex_float32" else np.complex128
    aux = {}

    def make(seed, dip):
        rng = np.random.default_rng(seed)
        x, aux["starts"], aux["payloads"] = build(case.settings, case.items, rng, dip)
        return case.settings, channel(x, rng, dtype=dt, **case.chan)
    s, x, mt, ct, co, m = tuned(make, list(case.feed), case.out_cap, seeds=seeds)
    return case, s, x, mt, ct, co, m, aux["starts"], aux["payloads"]


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/framesync.npz -> {case name: (stream, the calls of the reference's instantiation of the stream's own type, the
    integers() of its OTHER instantiation on the same stream)}: a call's labels are (kind, index, width, length or the phase), its
    state the estimates at the maximum as the reference held them after the call"""
    if not GOLDEN_PATH or not os.path.exists(GOLDEN_PATH):
        return {}
    g, out = np.load(GOLDEN_PATH), {}
    for k, name in enumerate(g["names"].tolist()):
        labels, phases, at, pat, oat, calls = g["labels%d" % k].tolist(), g["phases%d" % k].tolist(), 0, 0, 0, []
        for (consumed, produced, reserve, nl), est in zip(g["calls%d" % k].tolist(), g["est%d" % k].tolist()):
            ls = []
            for kind, index, width, length in labels[at:at + nl]:
                ls.append((LABEL_KINDS[kind], index, width, phases[pat] if kind == 0 else length))
                pat += kind == 0
            at += nl
            calls.append(Call(consumed, produced, reserve, ls, g["out%d" % k][oat:oat + produced], dict(scale=est[0], delta_fc=est[1], phase_off=est[2])))
            oat += produced
        olabels, at, other = g["other_labels%d" % k].tolist(), 0, []
        for consumed, produced, reserve, nl in g["other_calls%d" % k].tolist():
            other.append((consumed, produced, reserve, [(LABEL_KINDS[kind], index, width, None if kind == 0 else length) for kind, index, width, length in olabels[at:at + nl]]))
            at += nl
        out[name] = (g["x%d" % k], calls, other)
    return out


def integers(calls):
    """what a recorded call holds exactly: consumed, produced, reserve and the labels' kinds, indices, widths and lengths"""
    return [(c.consumed, c.produced, c.reserve, [(l[0], l[1], l[2], l[3] if l[0] != "phase_offset" else None) for l in c.labels]) for c in calls]


@functools.lru_cache(maxsize=None)
def prepared(name):
    """a case of CASES, computed once and shared by the tests that need it: on the recorded stream with the recorded reference's calls
    where tests/golden/framesync.npz holds the case, else as prepare() makes it.  The condition of the parity contract is asserted
    here, before anything is compared: the margins, and that the float reference, the double reference, the restatement and the truth
    agree on every integer."""
    case = next(c for c in CASES if c.name == name)
    if name not in golden():
        return prepare(case)
    x, ref, other = golden()[name]
    own, truth = (np.float32, np.float64) if x.dtype == np.complex64 else (np.float64, np.longdouble)
    mt, mo = Model(case.settings, truth, x), Model(case.settings, own, x)
    ct, co = mt.run(list(case.feed), case.out_cap), mo.run(list(case.feed), case.out_cap)
    ok_t, m_t = condition(mt.margins)
    ok_o, m_o = condition(mo.margins)
    assert ok_t and ok_o, (name, m_t, m_o)
    assert integers(ref) == other == integers(ct) == integers(co), name
    return case, case.settings, x, mt, ct, ref, tuple(min(a, b) for a, b in zip(m_t, m_o)), None, None


def seam_case(dtype, tile, peak, n=None):
    """a stream of n (3 * tile + 37) elements whose frame has its correlation peak at offset `peak`"""
    sw, dw, P = 6, 2, 5
    F = sw * dw * P + HEADER_BITS * dw
    n = 3 * tile + 37 if n is None else n
    return _case("seam_%d" % peak, dtype, sw, dw, P, [("gap", peak), ("frame", 6), ("gap", n - peak - F - 6 * dw)], mode="PHASE")


def value_errors(calls, truth, u):
    """the figures of the parity contract of one run against the truth's calls: per frame the payload error max|got - truth| /
    max|truth|, and at every call that finds a frame the errors of scale (relative), deltaFc and the phase label (wrapped).
    calls and truth: [Call] of the same schedule with equal decisions.  -> [(what, figure, floor)] with floor = 8 u s"""
    out, got, ref = [], [], []

    def flush():
        if ref:
            g, r = np.concatenate(got), np.concatenate(ref)
            out.append(("payload", float(np.max(np.abs(g.astype(np.clongdouble) - r)) / np.max(np.abs(r))), 8 * u))
        got.clear()
        ref.clear()
    for c, t in zip(calls, truth):
        if t.labels:
            flush()
            out.append(("scale", float(abs(np.longdouble(c.state["scale"]) - t.state["scale"]) / t.state["scale"]), 8 * u))
            out.append(("delta_fc", float(abs(np.longdouble(c.state["delta_fc"]) - t.state["delta_fc"])), 8 * u * np.pi))
            ph = [l[3] for l in c.labels if l[0] == "phase_offset"], [l[3] for l in t.labels if l[0] == "phase_offset"]
            if ph[1]:
                d = float(np.longdouble(ph[0][0]) - ph[1][0])
                out.append(("phase", abs((d + np.pi) % (2 * np.pi) - np.pi), 8 * u * np.pi))
        if t.produced:
            got.append(np.asarray(c.out))
            ref.append(np.asarray(t.out).astype(np.clongdouble))
    flush()
    return out


def within_bars(dev_errors, ref_errors):
    """every figure of the device within 2 max(E_ref, 8 u s) -> the list of (what, figure, bar, ratio) and whether all hold"""
    assert [w for w, _, _ in dev_errors] == [w for w, _, _ in ref_errors], "the two runs do not yield the same figures"
    rows = [(w, e, 2 * max(r, fl), e / (2 * max(r, fl))) for (w, e, fl), (_, r, _) in zip(dev_errors, ref_errors)]
    return rows, all(e <= bar for _, e, bar, _ in rows)
