"""CPU suite of /comms/wave_trigger: the model (tests/trigger_model.py) against the calls recorded from the reference
(tests/golden/trigger.npz, written by tests/golden/make_trigger_golden.py), the message and packet surface of the bundled runtime, and
the block's host logic that needs no device, through the runner: the setters and what they refuse, message forwarding, a dropped
buffer, the modes that never search, and the label trigger up to its capture."""
import os
import re

import numpy as np
import pytest

import trigger_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return M.load_golden()


@pytest.fixture(scope="module")
def blocks(pcx):
    from pothoscomms_amd import blocks as b
    b.load("trigger")
    return b


def make(blocks, nports=1):
    blk = blocks.make("/comms/wave_trigger", None, module="trigger")
    if nports > 1:
        blk.call("setNumPorts", nports)
    return blk


def drive(blocks, case, streams):
    """the case on the real block, the streams in host memory"""
    blk = make(blocks, len(case.dtypes))
    addrs = [s.ctypes.data for s in streams]
    return M.flatten(M.run_calls(case, streams, M.block_work(blk, streams, addrs, blocks.Label), M.block_call(blk), blk.activate))


# ---- the model against the reference's recorded calls: every integer, every label, every byte, position and level bit for bit
def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(c.name for c in M.CASES)
    assert os.path.getsize(M.GOLDEN_PATH) < max(os.path.getsize(os.path.join(os.path.dirname(M.GOLDEN_PATH), f))
                                                for f in os.listdir(os.path.dirname(M.GOLDEN_PATH)) if f.endswith(".npz") and f != "trigger.npz")


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_model_equals_the_recorded_reference(golden, case):
    streams, ref = golden[case.name]
    got = M.flatten(M.model_calls(case, streams))
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (case.name, k)


def test_the_recorded_cases_reach_what_they_are_for(golden):
    def packets(name):
        return [m for c in golden[name][1] for m in c[3] if m[0] == "packet"]

    def position(m):
        return float(np.uint64(m[2]).view(np.float64))

    for name in ("normal_pos_f32", "normal_neg_i16", "normal_level_u8", "complex_f32_pos", "complex_i16_level", "normal_pos_f64"):
        ps = packets(name)
        assert len(ps) >= 3 and all(("T", 4 if name != "normal_pos_f64" else 0, 1) in m[6] for m in ps), name
    assert any(position(m) != int(position(m)) for m in packets("normal_pos_f32"))          # a fraction
    # forced triggers carry position itself and no "T"
    assert all(position(m) == 4.0 and not m[6] for m in packets("automatic_forced") + packets("periodic"))
    assert not packets("disabled") and not packets("automatic_slow")
    # two windows: later windows were searched although the timer had not expired (the rate was 1e-3 from call 2 on)
    two = packets("semiautomatic_two_windows")
    assert len(two) >= 2 and all(len(m[5]) == 32 * 4 for m in two) and any(len([l for l in m[6] if l[0] == "T"]) == 2 for m in two)
    forced = packets("semiautomatic_forced_window")
    assert len(forced) == 1 and [l[0] for l in forced[0][6]] == ["T"]                          # the second window came from the timer
    # y1 == level: the crossing is consumed up to its SECOND element
    assert [position(m) for m in packets("second_equals_level")][:2] == [4.0, 4.0]
    assert len(packets("nan_pair")) == 1
    assert len(packets("two_ports_aligned")) % 2 == 0 and {m[4] for m in packets("two_ports_aligned")} == {"float32", "int16"}
    lab = [m for c in golden["label_trigger"][1] for m in c[3] if m[0] == "label"]
    assert {m[1] for m in lab} == {"rate", "go"} and all(not any(l[0] == "T" for l in m[6]) for m in packets("label_trigger"))
    msgs = [m for c in golden["messages"][1] for m in c[3]]
    assert ("label", "hello", 7, 1) in msgs and [m[4] for m in msgs if m[0] == "packet" and m[2] is None] == ["int16", "uint8"]
    assert any(c[1] != [-1] and c[1] != [0] for c in golden["hold_off_longer_than_a_call"][1])
    assert len(packets("set_hold_off_while_holding")) > len(packets("hold_off_longer_than_a_call"))


# ---- the search of the model itself
def test_model_search_edges():
    y = np.zeros(10, np.float32)
    y[4], y[5] = 0.25, 0.5
    assert M.search(y, 0.5, "POS", 0)[0] == 4 and M.position_of(4, y[4], y[5], 0.5) == 5.0
    assert M.search(y, 0.5, "POS", 5) is None and M.search(y, 0.5, "NEG", 0) is None
    y[6] = np.nan
    assert M.search(y, 0.5, "LEVEL", 5) is None
    big = np.array([0, 16777217, 16777219, 0], np.int64)
    assert M.search(M.search_floats(big, "int64"), 16777216.5, "POS", 0)[0] == 1                # 2^24 + 1 rounds below the level
    z = np.array([[3, 4], [30, 40]], np.int16)
    assert list(M.search_floats(z, "complex_int16")) == [5.0, 50.0]


# ---- the runner ABI: declared equals exported, in every module that links the runner
def test_trigger_module_exports_the_runner_abi():
    import subprocess
    src = open(os.path.join(ROOT, "include", "pcx_blocks.h")).read()
    declared = sorted(set(re.findall(r"PCXB_API\s+[\w\s\*]+?\b(pcxb_\w+)\s*\(", src)))
    for must in ("pcxb_plant_dtype", "pcxb_queue_packet", "pcxb_queue_label", "pcxb_work_inputs", "pcxb_message_count", "pcxb_message_info",
                 "pcxb_message_payload", "pcxb_message_labels", "pcxb_messages_clear", "pcxb_call_strings"):
        assert must in declared
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "pothoscomms_amd", "libpcx_trigger_blocks.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("pcxb_"))
    assert exported == declared


def test_registry_and_calls(blocks):
    assert blocks.module_registry_paths("trigger") == ["/blocks/wave_trigger", "/comms/wave_trigger"]
    assert blocks.registry_arity("/comms/wave_trigger", "trigger") == 0
    blk = make(blocks)
    calls = blk.calls()
    for name in ("setNumPorts", "setNumPoints", "setNumWindows", "setEventRate", "setAlignment", "setSource", "setHoldOff", "setSlope", "setMode", "setLevel",
                 "setPosition", "setLabelId", "setIdsList", "setDevice", "setPortSlabBytes"):
        assert calls[name] == 1, name
    for name in ("getNumPoints", "getNumWindows", "getEventRate", "getAlignment", "getSource", "getHoldOff", "getSlope", "getMode", "getLevel", "getPosition",
                 "getLabelId", "getDevice", "getPortSlabBytes"):
        assert calls[name] == 0, name
    # the block's description names calls that exist
    text = open(os.path.join(ROOT, "pothoscomms_amd", "csrc", "blocks", "trigger_blocks.cpp")).read()
    doc = text[text.index("|PothosDoc Wave Trigger"):text.index("class WaveTrigger")]
    named = re.findall(r"\|(?:setter|initializer) (\w+)\(", doc)
    assert len(named) == 14 and all(n in calls for n in named)
    assert "|factory /comms/wave_trigger()" in doc and "|alias /blocks/wave_trigger" in doc


def test_constructor_values_setters_and_what_they_refuse(blocks, pcx):
    blk = make(blocks)
    assert (blk.call("getNumPoints"), blk.call("getNumWindows"), blk.call("getEventRate"), blk.call("getAlignment")) == (1024, 1, 1.0, True)
    assert (blk.call("getSlope"), blk.call("getMode"), blk.call("getLevel"), blk.call("getPosition"), blk.call("getLabelId")) == ("POS", "AUTOMATIC", 0.5, 128, "")
    # the reference's getHoldOff and getSource return bool
    assert blk.call("getHoldOff") is True and blk.call("getSource") is False
    blk.call("setHoldOff", 0)
    assert blk.call("getHoldOff") is False
    blk.call("setNumPorts", 3)
    assert len(blk.ports(0)) == 3 and all(p[1] == "unspecified" for p in blk.ports(0))
    blk.call("setSource", 2)
    assert blk.call("getSource") is True
    for name, bad, words in (("setNumPoints", 0, "num points must be positive"), ("setNumWindows", 0, "num windows must be positive"),
                             ("setEventRate", 0.0, "event rate must be positive"), ("setEventRate", -1.0, "event rate must be positive"),
                             ("setSource", 3, "channel out of range"), ("setSlope", "UP", "unknown slope setting"), ("setMode", "ONCE", "unknown mode setting")):
        with pytest.raises(pcx._lib.InvalidArgument, match=words):
            blk.call(name, bad)
    assert (blk.call("getNumPoints"), blk.call("getNumWindows")) == (1024, 1)
    blk.call("setNumWindows", 4)
    blk.call("setLabelId", "go")
    blk.call("setIdsList", ["a", "b"])
    blk.call("setIdsList", [])
    assert (blk.call("getNumWindows"), blk.call("getLabelId")) == (4, "go")
    assert blk.buffer_manager(0)[0] == "circular"
    with pytest.raises(pcx._lib.InvalidArgument):
        blk.call("setPortSlabBytes", 1)


def test_messages_pass_through_and_an_untyped_packet_is_dropped(blocks):
    blk = make(blocks, 2)
    blk.call("setMode", "DISABLED")
    blk.call("setPosition", 2)
    blk.activate()
    blk.queue_packet(1, np.arange(6, dtype=np.int16), "int16", [blocks.Label("a", 2, 7), blocks.Label("b", 5, "s")], {"index": 9, "level": 2.5, "note": "x"})
    blk.queue_label(0, blocks.Label("rate", 3, 1e6))
    blk.queue_packet(0, np.arange(4, dtype=np.uint8), "", [])
    x = np.zeros(8, np.float32)
    blk.plant_dtype(0, "float32")
    blk.plant_dtype(1, "float32")
    consumed, reserve, yielded = blk.work_inputs([x.ctypes.data, x.ctypes.data], [8, 8])
    assert consumed == [20, 20] and reserve == [None, None] and not yielded          # 8 - position - 1 elements, in bytes
    got = blk.messages()
    assert [k for k, _ in got] == ["label", "packet"]                                # port 0's messages first; its packet had no type
    assert got[0][1] == blocks.Label("rate", 3, 1e6)
    m = got[1][1]
    assert (m.index, m.position, m.level, m.dtype) == (1, None, 2.5, "int16")        # "index" is overwritten with the port
    assert m.payload.view(np.int16).tolist() == list(range(6)) and m.labels == [blocks.Label("a", 2, 7), blocks.Label("b", 5, "s")]
    assert blk.messages() == []


def test_a_buffer_without_a_type_is_dropped_whole(blocks):
    blk = make(blocks)
    blk.call("setMode", "DISABLED")
    blk.activate()
    x = np.zeros(40, np.uint8)
    blk.plant_dtype(0, "")
    assert blk.work_inputs([x.ctypes.data], [40])[0] == [40]
    blk.plant_dtype(0, "int16")
    blk.call("setPosition", 100)
    assert blk.work_inputs([x.ctypes.data], [20]) == ([0], [204], False)              # (position + 2) elements, in bytes


@pytest.mark.parametrize("name", ["disabled", "automatic_slow"])
def test_block_equals_the_recording_where_nothing_searches(blocks, golden, name):
    case = [c for c in M.CASES if c.name == name][0]
    streams, ref = golden[name]
    assert drive(blocks, case, streams) == ref


def test_label_trigger_up_to_the_capture(blocks, golden):
    """the trigger comes from a label: host code alone.  The first call of the recorded case finds the label behind `position`, consumes
    up to `position` in front of it and yields; labels in front of it that were asked for leave as messages"""
    case = [c for c in M.CASES if c.name == "label_trigger"][0]
    streams, ref = golden["label_trigger"]
    blk = make(blocks)
    for name, value in case.settings:
        blk.call(name, value)
    blk.activate()
    work = M.block_work(blk, streams, [streams[0].ctypes.data], blocks.Label)
    labels = [(lid, at * 4, 4) for at, lid in case.labels[0] if at < case.feed[0]]
    got = M.flatten([work([(streams[0][:case.feed[0]], "float32")], [labels], [[]])])[0]
    assert got == ref[0]
    assert got[0] == [(50 - 4) * 4] and got[2] is True and got[3] == [("label", "go", 8, 4), ("label", "rate", 68, 4)]
    # the reserve a window asks for when the buffer is shorter than it: no device needed either
    assert blk.work_inputs([streams[0].ctypes.data], [10]) == ([0], [32 * 4], False)
