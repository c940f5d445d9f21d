"""Plain restatement of /comms/wave_trigger (utility/WaveTrigger.cpp of the reference): the level search, the work() state machine with
the clock replaced by a predicate, and the cases that tests/golden/make_trigger_golden.py records from the reference itself
(tests/golden/trigger.npz).  numpy float32 / float64 throughout, so that every quotient has the reference's bits.

A stream is a numpy array of the scalar type: (n,) for a real type, (n, 2) for a complex one.  A port without a type counts in BYTES:
consumed, reserve and the indices and widths of the labels on the port are bytes; the labels of a packet are elements of its payload.

The clock.  The reference asks two questions of its clock: has 1 / eventRate passed since the last trigger, and has 1.5 / eventRate.  The
recorded cases use eventRate = 1e9 (a nanosecond has always passed: both yes) or 1e-3 (both no), switched by the setter between calls.
The model answers both from `self.passed`, which set_event_rate sets from the rate the same way."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_PATH = os.path.join(HERE, "golden", "trigger.npz")

NP_OF = {"float64": np.float64, "float32": np.float32, "int64": np.int64, "int32": np.int32, "int16": np.int16, "int8": np.int8,
         "uint64": np.uint64, "uint32": np.uint32, "uint16": np.uint16, "uint8": np.uint8}
FAST, SLOW = 1e9, 1e-3


def is_complex(dtype):
    return dtype.startswith("complex_")


def np_scalar(dtype):
    return np.dtype(NP_OF[dtype[8:] if is_complex(dtype) else dtype])


def elem_bytes(dtype):
    return np_scalar(dtype).itemsize * (2 if is_complex(dtype) else 1)


def search_floats(x, dtype):
    """the stream as the float32 values the search looks at: static_cast<float> per component; a complex element becomes
    std::abs(std::complex<float>) = glibc's hypotf = (float)sqrt((double)a * a + (double)b * b) behind the infinite cases"""
    with np.errstate(all="ignore"):
        f = np.asarray(x).astype(np.float32)
        if not is_complex(dtype):
            return f
        a, b = f[:, 0].astype(np.float64), f[:, 1].astype(np.float64)
        y = np.sqrt(a * a + b * b).astype(np.float32)
        y[np.isinf(f[:, 0]) | np.isinf(f[:, 1])] = np.float32(np.inf)
        return y


def position_of(i, y0, y1, level):
    """i + (level - y0) / (y1 - y0): y1 - y0 a float32 subtraction, the rest float64 (WaveTrigger.cpp:747)"""
    with np.errstate(all="ignore"):
        dy = np.float32(np.float32(y1) - np.float32(y0))
        return float(np.float64(i) + (np.float64(level) - np.float64(y0)) / np.float64(dy))


def search(y, level, slope, start):
    """y: float32.  The least i in [start, len(y) - 2] whose pair triggers -> (i, y0, y1) or None"""
    if len(y) < 2 or start > len(y) - 2:
        return None
    a, b = y[:-1].astype(np.float64), y[1:].astype(np.float64)
    with np.errstate(invalid="ignore"):
        pos, neg = (a < level) & (b >= level), (a > level) & (b <= level)
    hit = pos if slope == "POS" else neg if slope == "NEG" else (pos | neg)
    hit[:start] = False
    at = np.flatnonzero(hit)
    if at.size == 0:
        return None
    i = int(at[0])
    return i, y[i], y[i + 1]


class Packet:
    def __init__(self):
        self.dtype, self.data, self.labels, self.meta = None, [], [], {}

    def elements(self):
        return sum(len(d) for d in self.data)


class Model:
    """work() of the reference, statement by statement.  A call takes, per port, (stream slice, dtype), the labels on it as (id, byte
    index, byte width) and the queued messages, and returns (consumed bytes per port, reserve per port or None, yielded, messages):
    a message is ("packet", index, position, level, dtype, payload bytes, [(id, index, width)]), ("label", id, index, width) or
    ("other",)."""

    def __init__(self, nports=1):
        self.nports = nports
        self.num_points, self.num_windows, self.alignment, self.source, self.hold_off = 1024, 1, True, 0, 1024
        self.slope, self.level, self.position, self.label_id, self.ids = "POS", 0.5, 128, "", set()
        self.points_remaining = self.windows_remaining = self.hold_off_remaining = 0
        self.event_offset, self.from_level = 0.0, False
        self.packets = []
        self.set_mode("AUTOMATIC")
        self.set_event_rate(1.0)

    # ---- the setters a case uses, by the block's own names ----
    def call(self, name, value):
        getattr(self, {"setNumPoints": "set_num_points", "setNumWindows": "set_num_windows", "setEventRate": "set_event_rate", "setAlignment": "set_alignment",
                       "setSource": "set_source", "setHoldOff": "set_hold_off", "setSlope": "set_slope", "setMode": "set_mode", "setLevel": "set_level",
                       "setPosition": "set_position", "setLabelId": "set_label_id", "setIdsList": "set_ids"}[name])(value)

    def set_num_points(self, v):
        if v == 0:
            raise ValueError("num points must be positive")
        self.num_points = int(v)

    def set_num_windows(self, v):
        if v == 0:
            raise ValueError("num windows must be positive")
        self.num_windows = int(v)

    def set_event_rate(self, v):
        if v <= 0.0:
            raise ValueError("event rate must be positive")
        self.event_rate = float(v)
        self.passed = v >= 1e6          # (FAST or SLOW; rates in between are not modelled)

    def set_alignment(self, v):
        self.alignment = bool(v)

    def set_source(self, v):
        if v >= self.nports:
            raise ValueError("channel out of range")
        self.source = int(v)

    def set_hold_off(self, v):
        self.hold_off = int(v)
        self.hold_off_remaining = min(self.hold_off_remaining, self.hold_off)

    def set_slope(self, v):
        if v not in ("POS", "NEG", "LEVEL"):
            raise ValueError("unknown slope setting")
        self.slope = v

    def set_mode(self, v):
        if v not in ("AUTOMATIC", "SEMIAUTOMATIC", "NORMAL", "PERIODIC", "DISABLED"):
            raise ValueError("unknown mode setting")
        self.mode = v
        self.window_timer = v == "SEMIAUTOMATIC"
        self.timer = v in ("AUTOMATIC", "PERIODIC")
        self.periodic = v == "PERIODIC"
        self.search_on = v in ("AUTOMATIC", "SEMIAUTOMATIC", "NORMAL")

    def set_level(self, v):
        self.level = float(v)

    def set_position(self, v):
        self.position = int(v)

    def set_label_id(self, v):
        self.label_id = v

    def set_ids(self, v):
        self.ids = set(v)

    def activate(self):
        self.points_remaining = self.windows_remaining = self.hold_off_remaining = 0
        self.packets = [Packet() for _ in range(self.nports)]

    # ---- work ----
    def work(self, bufs, labels=None, messages=None):
        n = self.nports
        labels = labels or [[] for _ in range(n)]
        messages = messages or [[] for _ in range(n)]
        self.consumed, self.reserve, self.yielded, self.out = [0] * n, [None] * n, False, []
        self._work(bufs, labels, messages)
        for p in range(n):                    # propagateLabels: the labels inside what was consumed, if their id was asked for
            for (lid, index, width) in labels[p]:
                if index < self.consumed[p] and lid in self.ids:
                    self.out.append(("label", lid, index, width))
        return self.consumed, self.reserve, self.yielded, self.out

    def _work(self, bufs, labels, messages):
        es = [elem_bytes(dt) if dt else 1 for _, dt in bufs]
        nbytes = [x.nbytes for x, _ in bufs]
        for p in range(self.nports):
            for m in messages[p]:
                if m[0] == "packet":          # ("packet", dtype or None, payload bytes, labels, has a type)
                    if m[1]:
                        self.out.append(("packet", p, None, None, m[1], bytes(m[2]), list(m[3])))
                else:
                    self.out.append(m)
            if nbytes[p] != 0 and not bufs[p][1]:
                self.consumed[p] += nbytes[p]
                return
        if self.points_remaining == 0:
            return self._trigger_work(bufs, labels, es, nbytes)

        W = self.num_points // self.num_windows
        first, last = self.windows_remaining == self.num_windows - 1, self.windows_remaining == 0
        all_acquired = True
        for p in range(self.nports):
            pk = self.packets[p]
            if pk.elements() // W + self.windows_remaining == self.num_windows:
                if not self.alignment:
                    self.consumed[p] += nbytes[p]
                continue
            x, dt = bufs[p]
            if len(x) < self.points_remaining:
                self.reserve[p] = self.points_remaining * es[p]
                all_acquired = False
                continue
            for (lid, index, width) in labels[p]:
                index, width = index // es[p], width // es[p]
                if index >= self.points_remaining:
                    break
                pk.labels.append((lid, index + pk.elements(), width))
            if self.from_level and p == self.source:
                pk.labels.append(("T", self.position + pk.elements(), 1))
            if first:
                pk.meta = dict(index=p, position=self.event_offset, level=self.level)
            self.consumed[p] += self.points_remaining * es[p] if self.alignment else nbytes[p]
            self.reserve[p] = 0
            pk.dtype = dt
            pk.data.append(np.ascontiguousarray(x[:self.points_remaining]))
        if not all_acquired:
            return
        if last:
            for p in range(self.nports):
                pk = self.packets[p]
                payload = b"".join(d.tobytes() for d in pk.data)
                self.out.append(("packet", pk.meta.get("index"), pk.meta.get("position"), pk.meta.get("level"), pk.dtype, payload, pk.labels))
                self.packets[p] = Packet()
        self.points_remaining = 0
        self.hold_off_remaining = self.hold_off

    def _trigger_work(self, bufs, labels, es, nbytes):
        src = self.source
        search_enabled = (self.windows_remaining > 0 or self.passed) and self.hold_off_remaining == 0
        num = len(bufs[src][0])
        ready = True
        for p in range(self.nports):
            if not self.alignment and p != src:
                self.consumed[p] += nbytes[p]
                continue
            num = min(num, len(bufs[p][0]))
            if num > self.position + 1:
                continue
            self.reserve[p] = (self.position + 2) * es[p]
            ready = False
        if not ready:
            return
        found, self.event_offset, self.from_level = False, float(self.position), False
        if search_enabled and self.search_on:
            if self.label_id:
                for (lid, index, _) in labels[src]:
                    if lid != self.label_id:
                        continue
                    index //= es[src]
                    if index < self.position:
                        continue
                    if index >= num - 1:
                        break
                    found, self.event_offset = True, float(index)
                    break
            else:
                hit = search(search_floats(bufs[src][0][:num], bufs[src][1]), self.level, self.slope, self.position)
                if hit:
                    found = self.from_level = True
                    self.event_offset = position_of(hit[0], hit[1], hit[2], self.level)
            if not found and (self.timer or (self.window_timer and self.windows_remaining != 0)):
                found = self.passed
        elif search_enabled and not self.search_on:
            found = self.timer
        if found:
            consume = int(self.event_offset - self.position)
            self.event_offset -= consume
        elif self.hold_off_remaining != 0:
            consume = min(num, self.hold_off_remaining)
            self.hold_off_remaining -= consume
        elif self.periodic:
            consume = num
        else:
            consume = num - self.position - 1
        for p in range(self.nports):
            if self.alignment or p == src:
                self.consumed[p] += consume * es[p]
        if found:
            if self.windows_remaining == 0:
                self.windows_remaining = self.num_windows
            self.windows_remaining -= 1
            self.points_remaining = self.num_points // self.num_windows
            self.reserve = [0] * self.nports
            self.yielded = True


# ---- the recorded cases ----
class Case:
    """name; dtypes, one per port; settings [(setter, value)] made before activate(); feed: call k offers every port feed[min(k, len - 1)]
    elements behind what it has consumed (or what is left); labels {port: [(element index in the stream, id)]}; events {call: [("set",
    setter, value) | ("packet", port, dtype or "", bytes) | ("label", port, id, index) | ("plant", port, dtype or "")]} carried out in
    front of that call; stream(rng, dtype, n) -> array"""

    def __init__(self, name, dtypes, settings, feed, n=480, labels=None, events=None, kind="sine", seed=1):
        self.name, self.dtypes, self.settings, self.feed, self.n = name, dtypes, settings, feed, n
        self.labels, self.events, self.kind, self.seed = labels or {}, events or {}, kind, seed


def make_stream(case, port):
    """the stream of one port of a case, chosen once by the maker (tests read it back from the fixture)"""
    dt = case.dtypes[port]
    rng = np.random.default_rng(1000 * case.seed + port)
    k = np.arange(case.n)
    if case.kind == "exact":                 # float32: a crossing whose second element IS the level, and one in front of the position
        y = np.zeros(case.n, np.float64)
        y[3:6] = [0.25, 0.5, 1.0]
        y[40:44] = [0.25, 0.5, 0.75, 0.0]
        y[90:93] = [0.125, 0.5, 0.5]
        y[200:204] = [0.3, 0.5, 0.2, 0.9]
        return y.astype(np_scalar(dt))
    if case.kind == "nan":                   # pairs with a NaN never trigger
        y = np.zeros(case.n, np.float64)
        y[20:26] = [0.0, np.nan, 1.0, np.nan, 0.0, 0.0]
        y[60:64] = [0.0, 0.4, 0.9, 0.0]
        return y.astype(np_scalar(dt))
    s = np.sin(2 * np.pi * k / 37.0 + 0.3 * port) + 0.2 * rng.standard_normal(case.n)
    sc = np_scalar(dt)
    amp, off = (1.0, 0.0) if sc.kind == "f" else (100.0, 128.0 if sc.kind == "u" else 0.0)
    if is_complex(dt):
        m = amp * (0.6 + 0.5 * s)
        ph = 2 * np.pi * rng.random(case.n)
        z = np.stack([m * np.cos(ph), m * np.sin(ph)], axis=1)
        return (z if sc.kind == "f" else np.round(z)).astype(sc)
    v = amp * s + off
    return (v if sc.kind == "f" else np.clip(np.round(v), np.iinfo(sc).min, np.iinfo(sc).max)).astype(sc)


def _base(mode, slope, level, rate=FAST, points=32, position=4, hold=8, windows=1):
    return [("setNumPoints", points), ("setNumWindows", windows), ("setEventRate", rate), ("setHoldOff", hold), ("setSlope", slope), ("setMode", mode),
            ("setLevel", level), ("setPosition", position)]


CASES = [
    Case("normal_pos_f32", ["float32"], _base("NORMAL", "POS", 0.25), [100, 37, 64]),
    Case("normal_neg_i16", ["int16"], _base("NORMAL", "NEG", -20.0), [64, 50]),
    Case("normal_level_u8", ["uint8"], _base("NORMAL", "LEVEL", 150.5), [90]),
    Case("normal_pos_f64", ["float64"], _base("NORMAL", "POS", -0.3, position=0, hold=0), [33, 70]),
    Case("automatic_forced", ["float32"], _base("AUTOMATIC", "POS", 50.0), [80]),
    Case("automatic_found", ["float32"], _base("AUTOMATIC", "POS", 0.1), [80, 45]),
    Case("automatic_slow", ["float32"], _base("AUTOMATIC", "POS", 0.1, rate=SLOW), [80]),
    Case("semiautomatic_two_windows", ["float32"], _base("SEMIAUTOMATIC", "POS", 0.2, windows=2), [70],
         events={2: [("set", "setEventRate", SLOW)], 9: [("set", "setEventRate", FAST)]}),
    Case("semiautomatic_forced_window", ["float32"], _base("SEMIAUTOMATIC", "POS", 0.2, windows=2), [70],
         events={2: [("set", "setLevel", 50.0)]}),
    Case("periodic", ["int16"], _base("PERIODIC", "POS", 0.0), [60]),
    Case("disabled", ["float32"], _base("DISABLED", "POS", 0.0), [60]),
    Case("complex_f32_pos", ["complex_float32"], _base("NORMAL", "POS", 0.8), [75, 40]),
    Case("complex_i16_level", ["complex_int16"], _base("NORMAL", "LEVEL", 60.0), [90]),
    Case("two_ports_aligned", ["float32", "int16"], _base("NORMAL", "POS", 0.25) + [("setAlignment", True)], [64, 40]),
    Case("two_ports_free", ["float32", "complex_int16"], _base("NORMAL", "POS", 0.25) + [("setAlignment", False), ("setSource", 1), ("setLevel", 60.0)],
         [64, 40]),
    Case("label_trigger", ["float32"], _base("NORMAL", "POS", 0.25) + [("setLabelId", "go"), ("setIdsList", ["rate", "go"])], [100, 41],
         labels={0: [(2, "go"), (17, "rate"), (50, "go"), (55, "other"), (130, "go"), (131, "rate"), (260, "go"), (300, "rate"), (470, "go")]}),
    Case("level_with_labels", ["int16"], _base("NORMAL", "POS", 10.0) + [("setIdsList", ["rate"])], [100, 41],
         labels={0: [(5, "rate"), (60, "x"), (61, "rate"), (62, "y"), (200, "rate"), (210, "x")]}),
    Case("messages", ["float32"], _base("NORMAL", "POS", 0.25), [64],
         events={0: [("packet", 0, "int16", 12), ("label", 0, "hello", 7)], 1: [("packet", 0, "", 8), ("packet", 0, "uint8", 5)], 3: [("plant", 0, "")],
                 4: [("plant", 0, "float32")]}),
    Case("second_equals_level", ["float32"], _base("NORMAL", "POS", 0.5, points=16, hold=2), [120], kind="exact"),
    Case("nan_pair", ["float32"], _base("NORMAL", "LEVEL", 0.5, points=16, hold=2), [100], kind="nan"),
    Case("hold_off_longer_than_a_call", ["float32"], _base("NORMAL", "POS", 0.25, hold=150), [50]),
    Case("set_hold_off_while_holding", ["float32"], _base("NORMAL", "POS", 0.25, hold=150), [50], events={4: [("set", "setHoldOff", 10)]}),
    Case("multi_window_reserve", ["int16", "float32"], _base("NORMAL", "NEG", 5.0, windows=4, points=64), [40, 12, 25]),
]


def message_payload(nbytes):
    """the payload of a packet a case queues on an input: nbytes bytes 1, 2, 3 ..."""
    return (np.arange(nbytes) + 1).astype(np.uint8)


MAX_CALLS = 400


def run_calls(case, streams, work, call, activate):
    """drives one block (the model, or the real one through `work`) through a case.  work(bufs, labels, messages) -> (consumed bytes,
    reserve, yielded, messages) with bufs [(slice, dtype)], labels [[(id, byte index, byte width)]], messages [[...]] per port;
    call(setter, value); activate().  Returns the list of what every call returned."""
    n = len(case.dtypes)
    for name, value in case.settings:
        call(name, value)
    activate()
    planted = list(case.dtypes)
    pos, out = [0] * n, []
    for k in range(MAX_CALLS):
        msgs = [[] for _ in range(n)]
        for ev in case.events.get(k, []):
            if ev[0] == "set":
                call(ev[1], ev[2])
            elif ev[0] == "plant":
                planted[ev[1]] = ev[2]
            elif ev[0] == "packet":
                msgs[ev[1]].append(("packet", ev[2], message_payload(ev[3]).tobytes(), [("m", 1, 1)]))
            else:
                msgs[ev[1]].append(("label", ev[2], ev[3], 1))
        feed = case.feed[min(k, len(case.feed) - 1)]
        bufs, labs, offered_all = [], [], True
        for p in range(n):
            es = elem_bytes(case.dtypes[p])
            m = min(feed, len(streams[p]) - pos[p])
            offered_all &= m == len(streams[p]) - pos[p]
            bufs.append((streams[p][pos[p]:pos[p] + m], planted[p]))
            labs.append([(lid, (at - pos[p]) * es, es) for at, lid in case.labels.get(p, []) if pos[p] <= at < pos[p] + m])
        consumed, reserve, yielded, posted = work(bufs, labs, msgs)
        out.append((list(consumed), list(reserve), bool(yielded), list(posted)))
        for p in range(n):
            assert consumed[p] % elem_bytes(case.dtypes[p]) == 0
            pos[p] += consumed[p] // elem_bytes(case.dtypes[p])
        if offered_all and not any(consumed) and not posted and not yielded and k + 1 > max(case.events, default=-1):
            break
    return out


def model_calls(case, streams):
    m = Model(len(case.dtypes))
    return run_calls(case, streams, m.work, m.call, m.activate)


# ---- the fixture ----
def bits(v):
    return None if v is None else int(np.float64(v).view(np.uint64))


def flatten(calls):
    """what every call did as plain integers, strings and bytes: comparable with ==, positions and levels as raw bits"""
    out = []
    for consumed, reserve, yielded, posted in calls:
        msgs = []
        for m in posted:
            if m[0] == "packet":
                msgs.append(("packet", m[1], bits(m[2]), bits(m[3]), m[4], bytes(m[5]), [tuple(l) for l in m[6]]))
            else:
                msgs.append(tuple(m))
        out.append((list(consumed), [-1 if r is None else r for r in reserve], bool(yielded), msgs))
    return out


def load_golden(path=None):
    """{name: (streams, flattened calls of the reference)}"""
    import json
    z = np.load(path or GOLDEN_PATH)
    out = {}
    for k, name in enumerate(z["names"]):
        case = [c for c in CASES if c.name == name][0]
        streams = [z["x%d_%d" % (k, p)] for p in range(len(case.dtypes))]
        pay = z["payload%d" % k].tobytes()
        calls = []
        for consumed, reserve, yielded, msgs in json.loads(str(z["calls%d" % k])):
            ms = []
            for m in msgs:
                if m[0] == "packet":
                    ms.append(("packet", m[1], m[2], m[3], m[4], pay[m[5]:m[5] + m[6]], [tuple(l) for l in m[7]]))
                else:
                    ms.append(tuple(m))
            calls.append((consumed, reserve, yielded, ms))
        out[str(name)] = (streams, calls)
    return out


# ---- the real block behind run_calls ----
def block_work(blk, streams, addrs, Label):
    """work(bufs, labels, messages) for run_calls on a /comms/wave_trigger made by pothoscomms_amd.blocks: port p's stream lies at address
    addrs[p] (host or device memory) with the bytes of streams[p]; Label is pothoscomms_amd.blocks.Label"""

    def work(bufs, labels, messages):
        for p, ms in enumerate(messages):
            for m in ms:
                if m[0] == "packet":
                    blk.queue_packet(p, np.frombuffer(m[2], np.uint8), m[1], [Label(l[0], l[1], None, l[2]) for l in m[3]])
                else:
                    blk.queue_label(p, Label(m[1], m[2], None, m[3]))
        ptrs, counts = [], []
        for p, (x, dt) in enumerate(bufs):
            blk.plant_dtype(p, dt)
            ptrs.append(addrs[p] + (x.ctypes.data - streams[p].ctypes.data if len(x) else 0))
            counts.append(len(x) if dt else x.nbytes)
        consumed, reserve, yielded = blk.work_inputs(ptrs, counts, [[Label(l[0], l[1], None, l[2]) for l in ls] for ls in labels])
        out = []
        for kind, m in blk.messages():
            if kind == "packet":
                out.append(("packet", m.index, m.position, m.level, None if m.dtype in ("", "unspecified") else m.dtype, m.payload.tobytes(),
                            [(l.id, l.index, l.width) for l in m.labels]))
            elif kind == "label":
                out.append(("label", m.id, m.index, m.width))
            else:
                out.append(("other",))
        return consumed, reserve, yielded, out

    return work


def block_call(blk):
    def call(name, value):
        blk.call(name, value)
    return call
