"""CPU suite of /comms/preamble_framer and /comms/frame_insert: the host planner (pcx_framer_plan, csrc/frame_plan.hpp) against the two
formulations of the model (tests/framer_model.py), its segment table executed on the host, the header coder with the model's decoder,
the C ABI's argument checks, the registry of libpcx_framer_blocks.so, the blocks' descriptions, defaults and refusals, and a stand-alone
sanitizer build of the planner run as a child process.  No device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import framer_model as M
from test_blockdocs_cpu import parse_docs, registered_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pothoscomms_amd", "csrc")
SRC = os.path.join(CSRC, "blocks", "framer_blocks.cpp")
REF = "/root/reference"
PATHS = ["/blocks/frame_insert", "/blocks/preamble_framer", "/comms/frame_insert", "/comms/preamble_framer"]
COMMON = {"setPreamble": 1, "getPreamble": 0, "setFrameStartId": 1, "getFrameStartId": 0, "setFrameEndId": 1, "getFrameEndId": 0,
          "setPaddingSize": 1, "getPaddingSize": 0, "setDevice": 1, "getDevice": 0, "setPortSlabBytes": 1, "getPortSlabBytes": 0}
INSERT_CALLS = dict(COMMON, setHeaderId=1, getHeaderId=0, setSymbolWidth=1, getSymbolWidth=0)
KIND = {"other": 0, "start": 1, "end": 2}
N = 40


def classify(label_id, start_id, end_id):
    """the blocks' rule: the start id is tested before the end id"""
    return "start" if label_id == start_id else "end" if label_id == end_id else "other"


def labelled(labels, start_id="frameStart", end_id="frameEnd"):
    """[(id, index, width)] -> events"""
    return [(index, width, classify(i, start_id, end_id), 0) for i, index, width in labels]


# the scenarios of the issue on 40 elements: name -> (events, padding)
SCENARIOS = {
    "reference": ([(5, 1, "start", 0), (33, 1, "end", 0)], 13),
    "index_0": ([(0, 1, "start", 7), (0, 1, "other", 0)], 13),
    "last_element": ([(39, 1, "start", 0), (39, 1, "end", 0)], 13),
    "beyond_the_buffer": ([(5, 1, "start", 0), (40, 1, "start", 0), (77, 1, "end", 0)], 13),
    "start_and_end_at_one_index": ([(7, 1, "start", 0), (7, 1, "end", 0), (9, 1, "other", 0)], 13),
    "end_and_start_at_one_index": ([(7, 1, "end", 0), (7, 1, "start", 0), (9, 1, "other", 0)], 13),
    "two_starts_at_one_index": ([(9, 1, "start", 1), (9, 1, "start", 2), (20, 1, "other", 0), (21, 1, "end", 0)], 13),
    "end_width_past_the_buffer": ([(30, 100, "end", 0)], 13),
    "end_width_overlaps_later_labels": ([(10, 8, "end", 0), (12, 1, "start", 3), (14, 1, "other", 0), (15, 2, "end", 0), (30, 1, "start", 0)], 5),
    "end_width_0": ([(10, 0, "end", 0), (12, 1, "other", 0)], 4),
    "equal_start_and_end_ids": (labelled([("x", 5, 1), ("x", 20, 1)], "x", "x"), 13),
    "empty_end_id_with_an_empty_id_label": (labelled([("frameStart", 5, 1), ("", 20, 1), ("else", 25, 1)], "frameStart", ""), 13),
    "padding_0": ([(5, 1, "start", 0), (33, 1, "end", 0), (35, 1, "other", 0)], 0),
    "no_labels": ([], 13),
    "others_only": ([(0, 1, "other", 0), (39, 1, "other", 0)], 13),
}
# (dtype, preamble, symbol width, header)
SETUPS = [("uint8", [0, 1, 1, 1, 1, 0], 1, False), ("complex_float32", [1, -1j, 0.5], 3, True), ("complex_float64", [1 + 2j], 2, False)]


def make(dev, setup, padding):
    dtype, pre, width, header = setup
    f = dev.Framer(dtype, pre, width, header, header_id=0xA7, padding=padding)
    sym, _, _ = f.preamble()
    return f, M.Config(M.rows(sym), width, header, 0xA7, padding)


def stream(dtype, n, seed=3):
    rng = np.random.default_rng(seed)
    if dtype == "uint8":
        return rng.integers(2, 256, n, dtype=np.uint8)
    return rng.standard_normal((n, 2)).astype(np.float32 if dtype == "complex_float32" else np.float64)


def run_table(x, segs, words, cfg):
    """the segment table executed on the host, as splice.hip reads it"""
    pool = np.repeat(cfg.preamble, cfg.width, axis=0)
    out = np.zeros((segs[-1][0], x.shape[1]), np.uint8)
    for (dst, kind, src), (end, _, _) in zip(segs[:-1], segs[1:]):
        assert end > dst
        ln = end - dst
        if kind == 0:
            assert src + ln <= x.shape[0]
            out[dst:end] = x[src:src + ln]
        elif kind == 1:
            assert src + ln <= pool.shape[0]
            out[dst:end] = pool[src:src + ln]
        elif kind == 2:
            assert src < len(words) and ln <= M.HEADER_BITS and cfg.header
            sym = cfg.preamble[-1]
            out[dst:end] = np.stack([sym if (words[src] >> k) & 1 else M.negated(sym) for k in range(ln)])
        else:
            assert kind == 3
    return out


def check_plan(f, cfg, x, events, cap):
    """the planner against both formulations; returns the walk's result"""
    xr = M.rows(x)
    a_out, a = M.walk(xr, events, cfg, cap)
    b_out, b = M.index_map(xr, events, cfg, cap)
    assert a[:6] == b[:6] and (a.error is None) == (b.error is None), (events, cap, a, b)
    eff = xr.shape[0] + len(events) * (M.insert_len(cfg) + cfg.padding) if cap is None else cap
    if a.error is not None:
        with pytest.raises(ValueError, match=r"need (\d+) output elements, the output buffer holds %d" % eff) as e:
            f.plan(xr.shape[0], eff, events)
        assert a.error in str(e.value)
        return a
    assert np.array_equal(a_out, b_out), (events, cap)
    res, segs, words = f.plan(xr.shape[0], eff, events)
    assert (res.consumed, res.out_len, res.cut, res.used_events) == (a.consumed, a.out_len, a.cut, sum(a.used)), (events, cap)
    assert list(res.used) == a.used, (events, cap)
    assert [int(v) if u else 0 for v, u in zip(res.insert_at, a.used)] == a.insert_at, (events, cap)
    assert [int(v) if u else 0 for v, u in zip(res.shift, a.used)] == a.shift, (events, cap)
    assert segs[-1] == (a.out_len, 3, 0) and all(s[0] < t[0] for s, t in zip(segs[:-1], segs[1:]))
    assert np.array_equal(run_table(xr, segs, words, cfg), a_out), (events, cap)
    assert all(events[i][0] < a.consumed for i in range(len(events)) if a.used[i])
    return a


@pytest.mark.parametrize("setup", SETUPS, ids=[s[0] for s in SETUPS])
def test_planner_equals_both_formulations_on_every_scenario(dev, setup):
    x = stream(setup[0], N)
    for name, (events, padding) in SCENARIOS.items():
        f, cfg = make(dev, setup, padding)
        a = check_plan(f, cfg, x, events, None)
        assert a.error is None and a.consumed == N and not a.cut, name
        f.close()


def test_the_references_own_scenario_gives_59_elements_and_labels_at_5_and_52(dev):
    f, cfg = make(dev, SETUPS[0], 13)
    events, _ = SCENARIOS["reference"]
    x = stream("uint8", N)
    a = check_plan(f, cfg, x, events, None)
    assert (a.consumed, a.out_len) == (40, 59) and M.expected_labels(events, a) == [(0, 5), (1, 33 + 6 + 13)]
    out, _ = M.walk(M.rows(x), events, cfg)
    want = np.concatenate([x[:5], [0, 1, 1, 1, 1, 0], x[5:34], np.zeros(13, np.uint8), x[34:]])
    assert np.array_equal(out.reshape(-1), want)
    f.close()


def test_the_oddities_of_the_references_loop(dev):
    f, cfg = make(dev, SETUPS[0], 13)
    x = stream("uint8", N)
    P = 6
    # two starts at one index insert twice and shift the later labels once
    ev, _ = SCENARIOS["two_starts_at_one_index"]
    a = check_plan(f, cfg, x, ev, None)
    assert a.insert_at[:2] == [9, 15] and a.shift == [0, 0, P, P + 13] and a.out_len == N + 2 * P + 13
    # the start id is tested first: with equal ids nothing is ever an end label
    ev, _ = SCENARIOS["equal_start_and_end_ids"]
    assert [e[2] for e in ev] == ["start", "start"] and check_plan(f, cfg, x, ev, None).out_len == N + 2 * P
    # an empty end id makes a label with an empty id an end label
    ev, _ = SCENARIOS["empty_end_id_with_an_empty_id_label"]
    assert [e[2] for e in ev] == ["start", "end", "other"]
    a = check_plan(f, cfg, x, ev, None)
    assert a.shift == [0, P + 13, P + 13] and a.out_len == N + P + 13
    # a label at or behind the end of the input is neither handled nor posted
    ev, _ = SCENARIOS["beyond_the_buffer"]
    assert check_plan(f, cfg, x, ev, None).used == [True, False, False]
    # an end label's head is clipped to the buffer, its padding comes behind the last element
    ev, _ = SCENARIOS["end_width_past_the_buffer"]
    a = check_plan(f, cfg, x, ev, None)
    assert a.insert_at == [N] and a.shift == [13] and a.out_len == N + 13
    f.close()
    # where this port differs: a head never runs backwards.  The end label at 10 passes 18 elements on; the start label at 12 inserts there
    f, cfg = make(dev, SETUPS[0], 5)
    ev, _ = SCENARIOS["end_width_overlaps_later_labels"]
    a = check_plan(f, cfg, x, ev, None)
    assert a.insert_at[:2] == [18, 23] and a.insert_at[3] == 29 and a.consumed == N
    f.close()


@pytest.mark.parametrize("setup", SETUPS[:2], ids=[s[0] for s in SETUPS[:2]])
def test_every_capacity_around_every_label(dev, setup):
    x = stream(setup[0], N)
    seen = {"cut": 0, "error": 0, "whole": 0}
    for name in ("reference", "start_and_end_at_one_index", "two_starts_at_one_index", "end_width_overlaps_later_labels", "index_0", "last_element",
                 "others_only"):
        events, padding = SCENARIOS[name]
        f, cfg = make(dev, setup, padding)
        full = M.walk(M.rows(x), events, cfg)[1].out_len
        for cap in range(0, full + 3):
            a = check_plan(f, cfg, x, events, cap)
            seen["error" if a.error else "cut" if a.cut else "whole"] += 1
            if not a.error:
                assert a.out_len <= cap and (a.cut or a.out_len == min(full, cap) or a.consumed < N)
        f.close()
    assert min(seen.values()) > 10, seen


def test_a_stream_cut_into_calls_by_a_small_buffer_equals_the_uncut_stream(dev):
    setup = SETUPS[1]
    x = stream(setup[0], 300, seed=8)
    events = [(0, 1, "start", 100), (40, 1, "other", 0), (99, 1, "end", 0), (100, 1, "start", 200), (100, 1, "other", 0), (250, 3, "end", 0), (299, 1, "other", 0)]
    f, cfg = make(dev, setup, 9)
    xr = M.rows(x)
    whole, w = M.walk(xr, events, cfg)
    want_labels = [at for _, at in M.expected_labels(events, w)]
    for cap in (M.insert_len(cfg) + 1, 71, 100, 128, 1000):
        pos, produced, outs, labels, left = 0, 0, [], [], list(events)
        while pos < xr.shape[0]:
            a = check_plan(f, cfg, x[pos:], left, cap)
            assert a.error is None and a.consumed > 0
            out, _ = M.walk(xr[pos:], left, cfg, cap)
            outs.append(out)
            labels += [produced + at for _, at in M.expected_labels(left, a)]
            pos, produced = pos + a.consumed, produced + a.out_len
            left = [(i - a.consumed, wd, k, ln) for (i, wd, k, ln), u in zip(left, a.used) if not u and i >= a.consumed]
        assert np.array_equal(np.concatenate(outs), whole) and labels == want_labels and not left, cap
    f.close()


def test_an_insert_larger_than_the_capacity_is_an_error_that_names_both_sizes(dev):
    f, cfg = make(dev, SETUPS[0], 13)
    with pytest.raises(ValueError, match=r"inserts at index 5 need 7 output elements, the output buffer holds 6"):
        f.plan(N, 6, [(5, 1, "start", 0)])
    assert f.plan(N, 7, [(5, 1, "start", 0)])[0].out_len == 5          # room for the insert, but first the five elements in front of it
    assert f.plan(N - 5, 7, [(0, 1, "start", 0)])[0].out_len == 7      # the preamble and the element the label sits on
    with pytest.raises(ValueError, match=r"need 14 output elements, the output buffer holds 13"):
        f.plan(N, 13, [(5, 1, "end", 0)])
    # two starts at one index are taken together or not at all
    with pytest.raises(ValueError, match=r"need 13 output elements, the output buffer holds 12"):
        f.plan(N, 12, [(5, 1, "start", 0), (5, 1, "start", 0)])
    f.close()


# ---- the header
@pytest.mark.parametrize("length", [0, 1, 0xFFF, 0x1000, 0xFFFF])
def test_header_decodes_to_what_was_encoded(dev, length):
    for header_id in (0x00, 0x55, 0xA7, 0xFF):
        word = dev.Framer.header_bits(header_id, length)
        assert word == M.header_word(header_id, length) and word >> M.HEADER_BITS == 0 and word & 3 == 2
        bits = [(word >> i) & 1 for i in range(M.HEADER_BITS)]
        got_id, got_len, got_chk, bad = M.header_decode(bits)
        # twelve bits of the length travel; the checksum covers all sixteen
        assert (got_id, got_len, bad) == (header_id, length & 0xFFF, False)
        assert got_chk == M.header_checksum(header_id, length)
        assert (got_chk == M.header_checksum(header_id, length & 0xFFF)) == (length < 0x1000 or M.header_checksum(header_id, length) == M.header_checksum(header_id, length & 0xFFF))
        # every single flipped bit of every Hamming word is corrected
        for i in range(2, M.HEADER_BITS):
            flipped = list(bits)
            flipped[i] ^= 1
            assert M.header_decode(flipped) == (header_id, length & 0xFFF, got_chk, False), i
        # two flipped bits in one word are reported
        flipped = list(bits)
        flipped[3] ^= 1
        flipped[8] ^= 1
        assert M.header_decode(flipped)[3]


def test_header_checksum_rotates_then_adds(dev):
    assert M.checksum8([0x55, 0, 0]) == 0x55 and M.checksum8([0x55, 1, 0]) == 0xD5 and M.checksum8([1, 1, 1]) == ((((0x80 + 1) >> 1) | 0x80) + 1) & 0xFF
    with pytest.raises(ValueError):
        dev.Framer.header_bits(256, 0)
    with pytest.raises(ValueError):
        dev.Framer.header_bits(0, 65536)


# ---- the C ABI (no device is touched)
def test_abi_argument_errors_come_before_any_device_call(pcx):
    L, E = pcx._lib.load(), pcx._lib.ERR_ARG
    buf = (C.c_double * 64)()
    plan = pcx._lib.FramePlan()
    ev = (pcx._lib.FrameEvent * 2)()
    h = C.c_void_p()
    assert L.pcx_framer_create(None, pcx._lib.U8, 0) == E
    for scalar, cplx in ((pcx._lib.U8, 1), (pcx._lib.F32, 0), (pcx._lib.F64, 0), (pcx._lib.I8, 0), (pcx._lib.I16, 1), (-1, 0), (10, 1)):
        assert L.pcx_framer_create(C.byref(h), scalar, cplx) == E and "unsupported type" in pcx._lib.last_error() and not h.value
    assert L.pcx_framer_set_preamble(None, buf, 1, 1, 0) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_framer_plan(None, 4, 4, None, 0, C.byref(plan), None, None, None, None, 0, None, 0) == E
    assert L.pcx_framer_process(None, buf, 4, None, 0, buf, 4, C.byref(plan), None, None, None) == E and "null handle" in pcx._lib.last_error()
    assert L.pcx_framer_process_dev(None, buf, 4, None, 0, buf, 4, C.byref(plan), None, None, None, None) == E
    tile, lds = C.c_size_t(), C.c_size_t()
    assert L.pcx_framer_get_geometry(None, C.byref(lds)) == E and L.pcx_framer_get_geometry(C.byref(tile), C.byref(lds)) == 0
    assert tile.value % 16 == 0 and tile.value >= 256 and lds.value >= 16
    assert L.pcx_frame_header_bits(0, 0, None) == E
    for scalar, cplx, es in ((pcx._lib.U8, 0, 1), (pcx._lib.F32, 1, 8), (pcx._lib.F64, 1, 16)):
        assert L.pcx_framer_create(C.byref(h), scalar, cplx) == 0
        try:
            n, w, hd, pad, hid = C.c_size_t(), C.c_size_t(), C.c_int(7), C.c_size_t(7), C.c_ubyte()
            assert L.pcx_framer_get_preamble(h, None, 0, C.byref(n), C.byref(w), C.byref(hd)) == 0 and (n.value, w.value, hd.value) == (1, 1, 0)
            assert L.pcx_framer_get_padding(h, C.byref(pad)) == 0 and pad.value == 0
            assert L.pcx_framer_get_header_id(h, C.byref(hid)) == 0 and hid.value == 0x55
            assert L.pcx_framer_set_preamble(h, buf, 0, 1, 0) == E and "preamble cannot be empty" in pcx._lib.last_error()
            assert L.pcx_framer_set_preamble(h, buf, 1, 0, 0) == E and "symbol width cannot be 0" in pcx._lib.last_error()
            assert L.pcx_framer_set_preamble(h, None, 1, 1, 0) == E
            assert (L.pcx_framer_set_preamble(h, buf, 1, 1, 1) == E) == (es == 1)
            assert L.pcx_framer_set_preamble(h, buf, 1 << 40, 1 << 40, 0) == E and "exceeds" in pcx._lib.last_error()
            # the checks of a call, in order: the plan, the events, the buffers, the overlap
            assert L.pcx_framer_process(h, buf, 4, None, 0, buf, 4, None, None, None, None) == E and "null plan" in pcx._lib.last_error()
            assert L.pcx_framer_process(h, buf, 4, None, 1, buf, 4, C.byref(plan), None, None, None) == E and "null events" in pcx._lib.last_error()
            assert L.pcx_framer_process(h, None, 4, ev, 0, buf, 4, C.byref(plan), None, None, None) == E and "null buffer" in pcx._lib.last_error()
            assert L.pcx_framer_process_dev(h, buf, 4, ev, 0, None, 4, C.byref(plan), None, None, None, None) == E and "null buffer" in pcx._lib.last_error()
            base = C.addressof(buf)
            for shift in (0, 1, 4 * es - 1, -(8 * es - 1)):
                for call in (lambda a, b: L.pcx_framer_process(h, a, 4, ev, 0, b, 8, C.byref(plan), None, None, None),
                             lambda a, b: L.pcx_framer_process_dev(h, a, 4, ev, 0, b, 8, C.byref(plan), None, None, None, None)):
                    assert call(C.c_void_p(base + 8 * es), C.c_void_p(base + 8 * es + shift)) == E and "overlaps" in pcx._lib.last_error()
            ev[0].kind = 3
            assert L.pcx_framer_plan(h, 4, 8, ev, 1, C.byref(plan), None, None, None, None, 0, None, 0) == E and "kind 3" in pcx._lib.last_error()
            ev[0].kind = 0
            # nothing to do
            assert L.pcx_framer_process(h, None, 0, None, 0, buf, 8, C.byref(plan), None, None, None) == 0 and plan.out_len == 0
            assert L.pcx_framer_process_dev(h, buf, 4, None, 0, None, 0, C.byref(plan), None, None, None, None) == 0 and plan.consumed == 0
        finally:
            assert L.pcx_framer_destroy(h) == 0
            h = C.c_void_p()


def test_header_declares_the_family_and_the_binding_covers_it(pcx):
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    family = sorted(set(re.findall(r"PCX_API\s+int\s+(pcx_frame\w+)\s*\(", src)))
    assert family == sorted(["pcx_frame_header_bits"] + ["pcx_framer_" + n for n in (
        "create", "destroy", "set_preamble", "get_preamble", "set_header_id", "get_header_id", "set_padding", "get_padding", "get_geometry", "plan",
        "process", "process_dev")])
    assert sorted(n for n in pcx._lib.SIGNATURES if n.startswith("pcx_frame")) == family
    out = subprocess.run(["nm", "-D", "--defined-only", pcx._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(family) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    # the structs of the binding are the header's
    assert (C.sizeof(pcx._lib.FrameEvent), C.sizeof(pcx._lib.FrameSegment), C.sizeof(pcx._lib.FramePlan)) == (24, 24, 48)


def test_device_handle_keeps_its_settings(dev):
    f = dev.Framer()
    sym, width, header = f.preamble()
    assert (sym.tolist(), width, header, f.header_id(), f.padding(), f.dtype) == ([1], 1, False, 0x55, 0, "uint8")
    f.set_preamble([3, 0, 255], 2)
    f.set_padding(11)
    assert f.preamble()[0].tolist() == [3, 0, 255] and f.preamble()[1] == 2 and f.padding() == 11
    with pytest.raises(ValueError):
        f.process(np.zeros(4, np.int8))
    f.close()
    f = dev.Framer("complex_float64", [1, -1, 1j], 20, True, header_id=3)
    sym, width, header = f.preamble()
    assert sym.tolist() == [[1, 0], [-1, 0], [0, 1]] and (width, header, f.header_id()) == (20, True, 3) and sym.dtype == np.float64
    f.close()
    for bad in ("float32", "int8", "complex_int16", "uint16"):
        with pytest.raises(ValueError):
            dev.Framer(bad)


# ---- the blocks (libpcx_framer_blocks.so)
def test_module_registry_holds_the_four_paths():
    from pothoscomms_amd import blocks as B
    assert B.module_registry_paths("framer") == PATHS
    for path in PATHS:
        assert B.registry_arity(path, module="framer") == (1 if "frame_insert" in path else 0)
        assert path not in B.registry_paths()
        for other in ("filter", "envelope", "iir", "digital", "correlator", "symbol", "repack", "waveform", "utility"):
            assert path not in B.module_registry_paths(other)


def test_a_fresh_preamble_framer_answers_the_constructors_values():
    from pothoscomms_amd import blocks as B
    for path in ("/comms/preamble_framer", "/blocks/preamble_framer"):
        b = B.make(path, module="framer")
        assert (b.in_dtype, b.out_dtype, b.in_dim, b.out_dim) == ("uint8", "uint8", 1, 1)
        assert b.calls() == COMMON
        assert (b.call("getPreamble"), b.call("getFrameStartId"), b.call("getFrameEndId"), b.call("getPaddingSize")) == ([1], "frameStart", "", 0)
        b.call("setPreamble", [0, 1, 1, 1, 1, 0])
        b.call("setFrameStartId", "go")
        b.call("setFrameEndId", "stop")
        b.call("setPaddingSize", 13)
        assert (b.call("getPreamble"), b.call("getFrameStartId"), b.call("getFrameEndId"), b.call("getPaddingSize")) == ([0, 1, 1, 1, 1, 0], "go", "stop", 13)
        with pytest.raises(ValueError, match="preamble cannot be empty"):
            b.call("setPreamble", [])
        assert b.call("getPreamble") == [0, 1, 1, 1, 1, 0]
        with pytest.raises(ValueError, match="64 KiB"):
            b.call("setPortSlabBytes", 1)
        assert b.call("getPortSlabBytes") == 64 << 20
        out, consumed, produced, reserve, labels = b.work(np.zeros(0, np.uint8), 64)          # no elements: nothing is consumed
        assert (out.size, consumed, produced, labels) == (0, 0, 0, [])
        b.close()


@pytest.mark.parametrize("dtype", ["complex_float32", "complex_float64"])
def test_a_fresh_frame_inserter_answers_the_constructors_values(dtype):
    from pothoscomms_amd import blocks as B
    for path in ("/comms/frame_insert", "/blocks/frame_insert"):
        b = B.make(path, dtype, module="framer")
        assert (b.in_dtype, b.out_dtype, b.in_dim, b.out_dim) == (dtype, dtype, 1, 1)
        assert b.calls() == INSERT_CALLS
        assert b.call("getPreamble").tolist() == [1] and (b.call("getFrameStartId"), b.call("getFrameEndId")) == ("frameStart", "frameEnd")
        assert (b.call("getHeaderId"), b.call("getSymbolWidth"), b.call("getPaddingSize")) == (0x55, 20, 0)
        b.call("setPreamble", [1, 1, -1, 0.25 - 0.5j])
        b.call("setHeaderId", 0xA7)
        b.call("setSymbolWidth", 3)
        b.call("setPaddingSize", 9)
        assert b.call("getPreamble").tolist() == [1, 1, -1, 0.25 - 0.5j]
        assert (b.call("getHeaderId"), b.call("getSymbolWidth"), b.call("getPaddingSize")) == (0xA7, 3, 9)
        with pytest.raises(ValueError, match="preamble cannot be empty"):
            b.call("setPreamble", [])
        with pytest.raises(ValueError, match="symbol width cannot be 0"):
            b.call("setSymbolWidth", 0)
        assert b.call("getSymbolWidth") == 3 and b.call("getPreamble").size == 4
        b.close()


@pytest.mark.parametrize("dtype", ["float32", "float64", "complex_int16", "complex_int32", "int8", "uint8"])
def test_an_unsupported_type_throws(dtype):
    from pothoscomms_amd import blocks as B
    for path in ("/comms/frame_insert", "/blocks/frame_insert"):
        with pytest.raises(ValueError, match="unsupported type"):
            B.make(path, dtype, module="framer")
    with pytest.raises(ValueError, match="unsupported type"):
        B.make("/comms/frame_insert", "complex_float32", dimension=2, module="framer")


EXT_PAIRS = {("device", "setDevice", "initializer"), ("portSlabBytes", "setPortSlabBytes", "initializer")}


def test_descriptions_match_the_registry_and_the_registered_calls():
    text = open(SRC).read()
    docs = parse_docs(text)
    assert [d["factory"] for d in docs] == [("/comms/preamble_framer", []), ("/comms/frame_insert", ["dtype"])]
    assert registered_calls(text) == set(INSERT_CALLS)
    common = {("preamble", "setPreamble", "setter"), ("frameStartId", "setFrameStartId", "setter"), ("frameEndId", "setFrameEndId", "setter"),
              ("paddingSize", "setPaddingSize", "setter")} | EXT_PAIRS
    want = [common, common | {("headerId", "setHeaderId", "setter"), ("symbolWidth", "setSymbolWidth", "setter")}]
    for d, pairs_want, calls in zip(docs, want, (COMMON, INSERT_CALLS)):
        pairs = set()
        for kind, fn, keys in d["calls"]:
            assert fn in calls and len(keys) == 1, fn
            pairs.add((keys[0], fn, kind))
        assert pairs == pairs_want
        assert set(d["params"]) == {k for k, _, _ in pairs} | set(d["factory"][1])
        assert d["category"] == ["/Digital"] and d["alias"] == [d["factory"][0].replace("/comms/", "/blocks/")]
        for p in d["params"].values():
            assert " ".join(p["desc"]).strip() and p["default"] is not None
        assert " ".join(d["prose"]).strip()
    assert docs[0]["params"]["frameEndId"]["default"] == '""' and docs[1]["params"]["frameEndId"]["default"] == '"frameEnd"'
    assert docs[1]["params"]["headerId"]["default"] == "0x55" and docs[1]["params"]["symbolWidth"]["default"] == "20"
    assert docs[0]["params"]["preamble"]["default"] == "[1]"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree exists in the build container only")
@pytest.mark.parametrize("which, ref_file", [(0, "PreambleFramer.cpp"), (1, "FrameInsert.cpp")])
def test_descriptions_have_the_reference_schema_and_their_own_words(which, ref_file):
    ours = parse_docs(open(SRC).read())[which]
    ref = parse_docs(open(os.path.join(REF, "digital", ref_file)).read())[0]
    assert ours["title"] == ref["title"] and ours["factory"] == ref["factory"] and ours["category"] == ref["category"]
    assert ours["alias"] == ref["alias"] and ours["keywords"] == ref["keywords"]
    ext = {"device", "portSlabBytes"}
    assert [k for k in ours["order"] if k not in ext] == ref["order"]
    assert {(fn, tuple(k), kind) for kind, fn, k in ours["calls"] if k[0] not in ext} == {(fn, tuple(k), kind) for kind, fn, k in ref["calls"]}
    for key, rp in ref["params"].items():
        for field in ("name", "default", "options", "widget", "preview", "tab", "units"):
            assert ours["params"][key][field] == rp[field], (key, field)

    def sentences(doc):
        text = " ".join(doc["prose"]) + " " + " ".join(" ".join(p["desc"]) for p in doc["params"].values())
        text = re.sub(r"<[^>]+>", " ", text)
        return {re.sub(r"\s+", " ", s).strip().lower() for s in re.split(r"[.;:]\s", text) if len(s.split()) >= 6}
    assert sentences(ours) and sentences(ref) and not (sentences(ours) & sentences(ref))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_source_type_checks_against_the_pothos_surface():
    blocks = os.path.dirname(SRC)
    flags = ["-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-DPCX_WITH_POTHOS",
             "-I" + os.path.join(ROOT, "tests", "pothos_decl"), "-I" + os.path.join(ROOT, "include"), "-I" + blocks]
    r = subprocess.run(["g++"] + flags + [SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_port_slab_default_is_the_one_of_the_other_modules():
    blocks = os.path.dirname(SRC)
    pat = r"constexpr size_t kPortSlabBytes = (\d+)u << (\d+);"
    a = re.search(pat, open(os.path.join(blocks, "comms_blocks.cpp")).read())
    b = re.search(pat, open(SRC).read())
    assert a and b and int(a.group(1)) << int(a.group(2)) == int(b.group(1)) << int(b.group(2))
    for d in parse_docs(open(SRC).read()):
        assert int(d["params"]["portSlabBytes"]["default"]) == int(a.group(1)) << int(a.group(2))


def test_the_module_library_exports_the_runner_and_nothing_of_the_blocks():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_framer_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"pcxb_make", "pcxb_work", "pcxb_call_bytes", "pcxb_get_bytes", "pcxb_call_taps", "pcxb_get_taps", "pcxb_call_size", "pcxb_registry_path"} <= exported
    assert all(s.startswith("pcxb_") for s in exported), sorted(s for s in exported if not s.startswith("pcxb_"))


# ---- the planner header on its own, under the sanitizers
def fnv(values):
    d = 1469598103934665603
    for v in values:
        d = ((d ^ (int(v) & 0xFFFFFFFFFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return d


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_planner_header_alone_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "framer_plan_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, os.path.join(ROOT, "tests", "framer_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # the scenarios above at every interesting capacity, in the program's own coding of the elements (input element i is i + 1,
    # sync word element j is -(j + 1), padding 0): rows of 8 bytes for the model
    x = (np.arange(N, dtype=np.int64) + 1).view(np.uint8).reshape(N, 8)
    cases, lines = [], []
    for sync in (6, 1, 17):
        pre = (-(np.arange(sync, dtype=np.int64) + 1)).view(np.uint8).reshape(sync, 8)
        for name, (events, padding) in SCENARIOS.items():
            cfg = M.Config(pre, 1, False, 0x55, padding)
            full = N + len(events) * (sync + padding)
            for cap in sorted({full, full // 2, sync, sync + 1, sync + padding + 2, 0, 1, 33}):
                cases.append((cfg, events, cap))
                lines.append(" ".join(str(v) for v in [N, cap, sync, 0, padding, len(events)] + [w for e in events for w in (e[0], e[1], KIND[e[2]], e[3])]))
    # with a header: the numbers only
    hdr_events, hdr_pad = SCENARIOS["end_width_overlaps_later_labels"]
    lines.append(" ".join(str(v) for v in [N, 4000, 6, 1, hdr_pad, len(hdr_events)] + [w for e in hdr_events for w in (e[0], e[1], KIND[e[2]], e[3])]))
    lines.append("random 7 4000")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    got = run.stdout.splitlines()
    assert len(got) == len(lines)
    for (cfg, events, cap), line in zip(cases, got):
        out, a = M.walk(x, events, cfg, cap)
        if a.error:
            assert line == "error framer: " + a.error, (events, cap, line)
            continue
        want = "%d %d %d %d | %s | %s | %s | %d" % (a.consumed, a.out_len, a.cut, sum(a.used), " ".join(str(int(u)) for u in a.used),
                                                   " ".join(str(v) for v in a.insert_at), " ".join(str(v) for v in a.shift),
                                                   fnv(np.ascontiguousarray(out).view(np.int64).reshape(-1)))
        assert re.sub(r"\s+", " ", line) == re.sub(r"\s+", " ", want), (events, cap)
    cfg = M.Config(np.zeros((6, 16), np.uint8), 1, True, 0x55, hdr_pad)
    a = M.walk(np.zeros((N, 16), np.uint8), hdr_events, cfg)[1]
    assert got[-2].startswith("%d %d 0 %d |" % (a.consumed, a.out_len, sum(a.used)))
    m = re.match(r"random 4000 plans, (\d+) errors, (\d+) cuts$", got[-1])
    assert m and int(m.group(2)) > 100, got[-1]


# ---- the recorded reference: tests/golden/framer.npz, what the reference's own work() posted (tests/golden/make_framer_golden.py)
GOLDEN = os.path.join(ROOT, "tests", "golden", "framer.npz")
# DESIGN.md 18, "a head never runs backwards": the recorded cases in which some start label's index, or some end label's index + width,
# lies in front of what earlier labels have passed on.  There, and nowhere else, model and reference may differ: the reference's
# `label.index - consumed` wraps.  An end label passes the element it sits on, so a start label behind it at the SAME index is such a case
BACKWARD = sorted(
    ["small/%s/%s" % (t, s) for t in M.GOLDEN_TYPES for s in ("end_width_overlaps_later_labels", "end_and_start_at_one_index")]
    + ["seam/%s/start_end_start_%s" % (t, w) for t in M.GOLDEN_TYPES for w in ("first", "before_seam", "seam", "last")]
    + ["backward/%s/ends_only" % t for t in M.GOLDEN_TYPES]
    + ["backward/uint8/start_behind_an_end", "backward/uint8/end_ends_in_front_of_a_start"])


@pytest.fixture(scope="module")
def golden():
    return M.golden_cases(GOLDEN)


def data_kind(data):
    return M.DATA_KINDS.index(None if data is None else "integer" if isinstance(data, int) else "string")


def posted_by(c, res):
    """what the blocks post by the model's result, as the recording has it: (place of the input label, index, width, kind of data)"""
    return [(k, at, c["labels"][k][2], data_kind(c["labels"][k][3])) for k, at in M.expected_labels(c["events"], res)]


def equals_the_recording(c, out, consumed, posted):
    return not c["leaves"] and consumed == c["consumed"] and posted == c["posted"] and out.shape == c["out"].shape and np.array_equal(out, c["out"])


def backward_labels(c):
    """the issue's rule, on the labels alone"""
    passed, found = 0, []
    for k, (index, width, kind, _) in enumerate(c["events"]):
        if index >= c["n"]:
            continue
        if kind == "start":
            found += [k] if index < passed else []
            passed = max(passed, index)
        elif kind == "end":
            found += [k] if index + width < passed else []
            passed = max(passed, min(index + width, c["n"]))
    return found


def test_both_formulations_equal_the_recorded_reference_except_on_the_backward_cases(golden):
    _, cases, _ = golden
    differ, ran = {"walk": [], "index_map": []}, 0
    for c in cases:
        for f in (M.walk, M.index_map):
            out, res = f(c["x"], c["events"], c["cfg"])
            assert res.error is None and not res.cut, c["name"]
            if not equals_the_recording(c, out, res.consumed, posted_by(c, res)):
                differ[f.__name__].append(c["name"])
        ran += 1
    assert ran == np.load(GOLDEN)["names"].size
    backward = sorted(c["name"] for c in cases if c["backward"])
    assert backward == sorted(c["name"] for c in cases if backward_labels(c))          # the maker's flag is the rule
    assert sorted(differ["walk"]) == sorted(differ["index_map"]) == backward == BACKWARD
    assert all(c["backward"] for c in cases if c["leaves"])


def test_planner_equals_the_recorded_reference_on_every_case_that_is_not_backward(dev, golden):
    _, cases, _ = golden
    ran = 0
    for c in cases:
        if c["backward"]:
            continue
        cfg = c["cfg"]
        f = dev.Framer(c["dtype"], c["preamble"], cfg.width, cfg.header, header_id=cfg.header_id, padding=cfg.padding)
        cap = c["n"] + len(c["events"]) * (M.insert_len(cfg) + cfg.padding)
        res, segs, words = f.plan(c["n"], cap, c["events"])
        posted = [(k, c["events"][k][0] + int(res.shift[k]), c["labels"][k][2], data_kind(c["labels"][k][3])) for k in range(len(c["events"])) if res.used[k]]
        assert not res.cut and res.out_len == c["out"].shape[0], c["name"]
        assert equals_the_recording(c, run_table(c["x"], segs, words, cfg), res.consumed, posted), c["name"]
        f.close()
        ran += 1
    assert ran == len(cases) - len(BACKWARD)


def test_on_the_backward_cases_a_head_never_runs_backwards(golden):
    """the backward label's head is empty, its insert goes where the output stands, and the input passes once, in order"""
    _, cases, _ = golden
    ran = 0
    for c in cases:
        if not c["backward"]:
            continue
        cfg, ev = c["cfg"], c["events"]
        out, res = M.walk(c["x"], ev, cfg)
        out2, res2 = M.index_map(c["x"], ev, cfg)
        assert np.array_equal(out, out2) and res[:6] == res2[:6] and res.consumed == c["n"] and all(res.used), c["name"]
        behind, stand, inserted = backward_labels(c), 0, np.zeros(out.shape[0], bool)
        assert behind
        for k, (index, width, kind, length) in enumerate(ev):
            if kind == "other":
                continue
            rows_k = M.insert_rows(cfg, length) if kind == "start" else np.zeros((cfg.padding, out.shape[1]), np.uint8)
            at = res.insert_at[k]
            assert at >= stand and (at == stand) >= (k in behind), (c["name"], k)
            assert np.array_equal(out[at:at + rows_k.shape[0]], rows_k), (c["name"], k)
            inserted[at:at + rows_k.shape[0]] = True
            stand = at + rows_k.shape[0]
        assert np.array_equal(out[~inserted], c["x"]), c["name"]
        ran += 1
    assert ran == len(BACKWARD)


def test_header_coder_and_decoder_equal_the_recorded_reference(dev, golden):
    import hashlib
    _, _, header = golden
    assert len(header["enc"]) == 256 * 6 and {ln for _, ln, _ in header["enc"]} == {0, 1, 0x0FFF, 0x1000, 0xABCD, 0xFFFF}
    for header_id, length, word in header["enc"]:
        assert sum(b << i for i, b in enumerate(M.header_bits(header_id, length))) == word == dev.Framer.header_bits(header_id, length), (header_id, length)
    assert sorted(header["enc_all"]) == [0x55, 0xA7]
    for header_id, sha in header["enc_all"].items():
        words = np.array([M.header_word(header_id, length) for length in range(65536)], dtype="<u8")
        assert hashlib.sha256(words.tobytes()).hexdigest() == sha, header_id
        assert np.array_equal(words, np.array([dev.Framer.header_bits(header_id, length) for length in range(65536)], dtype="<u8")), header_id
    # per (id, length): the clean word, every single flipped bit (corrected, or one of the two sync bits) and flips of two bits
    assert len(header["dec"]) == 6 * (1 + M.HEADER_BITS + 60 + 7)
    for word, header_id, length, chk, error in header["dec"]:
        assert M.header_decode([(word >> i) & 1 for i in range(M.HEADER_BITS)]) == (header_id, length, chk, bool(error)), hex(word)
    errors = sum(r[4] for r in header["dec"])
    assert len(header["dec"]) - errors >= 6 * (1 + M.HEADER_BITS) and errors >= 6 * 7 and max(r[2] for r in header["dec"]) <= 0xFFF


def test_recorded_framer_fixture_covers_what_it_is_meant_to(golden):
    tile_bytes, cases, header = golden
    assert os.path.getsize(GOLDEN) <= 512 << 10 and tile_bytes == 16384
    by = {c["name"]: c for c in cases}
    assert len(by) == len(cases)
    assert all(index < 1 << 31 for c in cases for _, index, _, _ in c["labels"])
    # the scenarios above, on every type, with the ids that make their kinds
    for t in M.GOLDEN_TYPES:
        for name, (events, padding) in SCENARIOS.items():
            c = by["small/%s/%s" % (t, name)]
            assert c["events"] == [(i, w, k, ln if k == "start" else 0) for i, w, k, ln in events] and c["cfg"].padding == padding and c["n"] == N, c["name"]
        assert (by["small/%s/equal_start_and_end_ids" % t]["start_id"], by["small/%s/equal_start_and_end_ids" % t]["end_id"]) == ("x", "x")
        c = by["small/%s/empty_end_id_with_an_empty_id_label" % t]
        assert c["end_id"] == "" and [l[0] for l in c["labels"]] == ["frameStart", "", "else"]
        # three tiles and 37 elements; labels on the last element of a tile, on the first of the next and on the stream's last
        tile = tile_bytes // c["x"].shape[1]
        seam = [c for c in cases if c["name"].startswith("seam/%s/" % t)]
        assert len(seam) == 20 and all(c["n"] == 3 * tile + 37 for c in seam)
        for at in (0, tile - 1, tile, 3 * tile + 36):
            for kind in ("start", "end"):
                assert any(e[0] == at and e[2] == kind for c in seam if not c["backward"] for e in c["events"]), (t, at, kind)
        assert by["seam/%s/insert_on_an_output_seam" % t]["posted"][1][:2] == (1, tile)      # an insert that begins on a seam of the output
    assert [by["unit/P%d" % p]["preamble"].size for p in (1, 15, 16, 17, 33)] == [1, 15, 16, 17, 33]
    for where in ("before_the_seam", "across_the_seam"):
        c = by["run64/" + where]
        idx = [e[0] for e in c["events"]]
        assert len(idx) == 64 and idx == list(range(idx[0], idx[0] + 64)) and (idx[0] + 128 < tile_bytes) == (where == "before_the_seam")
    # every kind of label and of label data is posted somewhere; the header's length field sees 0, 0xFFF, 0xABCD and a cut product
    kinds = {(e[2], p[3]) for c in cases if not c["leaves"] for p in c["posted"] for e in [c["events"][p[0]]]}
    assert kinds >= {(k, d) for k in ("start", "end", "other") for d in (0, 1, 2)}, kinds
    for t in M.GOLDEN_TYPES[1:]:
        negated_zero = 0
        for last in ("1_0", "0_m2", "m0_3", "0_0"):
            c = by["header/%s/%s" % (t, last)]
            assert {e[3] for e in c["events"] if e[2] == "start"} == {0, 0xFFF, 0xABCD, (70000 * 3) & 0xFFFF} and (70000 * 3) >> 16
            sym = c["cfg"].preamble[-1]
            half = sym.size // 2
            zero = [h for h in (0, 1) if not sym[h * half:(h + 1) * half].any()]        # components that are +0.0
            minus = M.negated(sym)
            assert (c["out"] == minus).all(axis=1).any() and (c["out"] == sym).all(axis=1).any()
            negated_zero += len(zero)
        assert negated_zero >= 3                                                          # (1, 0), (0, -2) and both of (0, 0)
    assert len(cases) == 3 * len(SCENARIOS) + 3 * 20 + 5 + 2 + 8 + 5 + 1
