"""CPU suite of /comms/frame_sync: the model (tests/framesync_model.py) against the recorded reference (tests/golden/framesync.npz),
the margin condition of the parity contract on every recorded stream, the header word the model reads from a clean frame, the setters
of the handle (no device is touched), and the host side of a search call -- Hamming decoder, checks, label arithmetic, the backing up of
the DEBUG mode -- as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import framer_model
import framesync_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pothoscomms_amd", "csrc")
SRC = os.path.join(CSRC, "blocks", "framesync_blocks.cpp")
U = {"complex_float32": 2.0 ** -24, "complex_float64": 2.0 ** -53}
NAMES = [c.name for c in M.CASES]


def test_the_fixture_holds_every_case():
    assert sorted(M.golden()) == sorted(NAMES)
    # sync words of more than one and more than two chunks of the search kernel's staging are among them, for both types
    assert sorted(M.derived(c.settings)[0] for c in M.CASES if "chunks" in c.name) == [1050, 1050, 1575, 1575]
    assert os.path.getsize(M.GOLDEN_PATH) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_model_against_the_recorded_reference(name):
    """decisions exact between the float reference, the double reference and the model; the recorded reference's values within the
    rounding bound of its own sums against the truth (the bars of the GPU suite are built from these figures)"""
    case, s, x, mt, ct, ref, margins = M.prepared(name)[:7]
    other = M.golden()[name][2]
    # the condition, before anything is compared: a cap, not a measurement
    assert margins[0] >= M.CAP_ENV and margins[1] >= M.CAP_INT and margins[2] >= M.CAP_BIT, margins
    assert M.integers(ref) == other == M.integers(ct)
    u = U[case.dtype]
    e_ref = M.value_errors(ref, ct, u)
    # the truth computes what the reference computes: the reference's own error is a rounding error, by the length of its sums
    # (W terms into L, F steps of the running angle) and no more
    W, F = M.derived(s)[:2]
    for what, e, floor in e_ref:
        assert e <= 8 * F * u * (np.pi if what in ("phase", "delta_fc") else 1), (what, e)
    if any(c.labels for c in ct):
        assert any(w == "scale" for w, _, _ in e_ref)


def test_frames_are_found_where_they_were_put():
    for name in ("raw_len19_5_3_p2", "back_to_back", "one_flip_then_far"):
        case, s, x, mt, ct = M.prepared(name)[:5]
        lengths = [l[3] for c in ct for l in c.labels if l[0] == "frame_start"]
        want = [it[1] for it in case.items if it[0] == "frame"]
        assert lengths == (want if name != "one_flip_then_far" else [3, 4])
    for name in ("wrong_id_then_near", "length_0_then_far", "two_flips_then_near"):
        ct = M.prepared(name)[4]
        assert [l[3] for c in ct for l in c.labels if l[0] == "frame_start"] == [4]
    for name in ("silence", "carrier", "below_threshold"):
        assert not any(c.labels or c.produced for c in M.prepared(name)[4])
    # the carrier correlates at every offset (its envelope gate is open) and declares nothing
    mt = M.prepared("carrier")[3]
    assert len(mt.peaks_seen) > 400 and max(L for _, L in mt.peaks_seen) < mt.mag


def test_a_call_without_a_frame_carries_the_count():
    ct = M.prepared("declared_next_call")[4]
    assert not ct[0].labels and ct[0].state["max_peak"] > 0 and 0 < ct[0].state["count_since_max"] < M.derived(M.prepared("declared_next_call")[1])[3]
    assert ct[1].labels


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_header_word_of_a_clean_frame(dtype):
    for sw, dw, P, hid, length in ((5, 3, 2, 0x55, 19), (8, 4, 3, 0xA7, 0xABC), (6, 2, 5, 0x00, 1)):
        s = M.settings(sw=sw, dw=dw, preamble=M.PRE[P], header_id=hid)
        x = np.concatenate([np.zeros(9), M.frame(s, length, M.qpsk(np.random.default_rng(1), 4), dip=0.0), np.zeros(M.derived(s)[1])]).astype(dtype)
        m = M.Model(s, np.float64, x)
        first, bits = m._header(9, np.float64(1), np.float64(0), np.float64(0))
        assert first == M.derived(s)[0] + dw // 2
        assert sum(b << i for i, b in enumerate(bits)) == framer_model.header_word(hid, length)
        assert framer_model.header_decode(bits) == (hid, length & 0xFFF, framer_model.header_checksum(hid, length), False)


def test_setters(dev):
    for dtype in ("complex_float32", "complex_float64"):
        fs = dev.FrameSync(dtype)
        for mode in M.MODES:
            fs.set_output_mode(mode)
            assert fs.output_mode() == mode
        for bad in ("raw", "", "SOFT"):
            with pytest.raises(ValueError, match="unknown output mode"):
                fs.set_output_mode(bad)
        with pytest.raises(ValueError, match="preamble cannot be empty"):
            fs.set_preamble([])
        for w in (0, 1):
            with pytest.raises(ValueError, match="at least 2 samples"):
                fs.set_data_width(w)
        with pytest.raises(ValueError, match="symbol width cannot be 0"):
            fs.set_symbol_width(0)
        for w in (1, 2):
            with pytest.raises(ValueError, match="at least 3 samples"):
                fs.set_symbol_width(w)
        with pytest.raises(ValueError, match="non-negative"):
            fs.set_input_threshold(-1e-9)
        # what was refused changed nothing
        assert (fs.output_mode(), fs.symbol_width(), fs.data_width(), fs.preamble().tolist()) == ("DEBUG", 20, 4, [[1.0, 0.0]])
        fs.set_input_threshold(0.0)
        fs.set_symbol_width(3)
        fs.set_data_width(2)
        fs.set_preamble([1, -1, 0.5j])
        fs.set_header_id(0x1A7)
        fs.set_verbose(True)
        assert fs.geometry()[:4] == (18, 18 + 58 * 2, 12, 9) and fs.header_id() == 0xA7 and fs.input_threshold() == 0.0
        assert fs.preamble().tolist() == [[1, 0], [-1, 0], [0, 0.5]]
    with pytest.raises(ValueError, match="unsupported type"):
        dev.FrameSync("float32")
    with pytest.raises(ValueError, match="unsupported type"):
        dev.FrameSync("complex_int16")


def test_abi_family_and_structs(pcx):
    import ctypes as C
    src = open(os.path.join(ROOT, "include", "pcx.h")).read()
    family = sorted(set(re.findall(r"PCX_API\s+int\s+(pcx_fsync_\w+)\s*\(", src)))
    assert len(family) == 21 and sorted(n for n in pcx._lib.SIGNATURES if n.startswith("pcx_fsync_")) == family
    assert (C.sizeof(pcx._lib.FsyncLabel), C.sizeof(pcx._lib.FsyncResult)) == (40, 32 + 3 * 40 + 64)
    L = pcx._lib.load()
    h, r = C.c_void_p(), pcx._lib.FsyncResult()
    assert L.pcx_fsync_create(C.byref(h), pcx.F32, 1) == 0
    assert L.pcx_fsync_set_output_mode(h, 4) == pcx._lib.ERR_ARG and L.pcx_fsync_set_label_id(h, 3, b"x") == pcx._lib.ERR_ARG
    assert L.pcx_fsync_process(None, None, 0, None, 0, C.byref(r)) == pcx._lib.ERR_ARG
    assert L.pcx_fsync_process(h, None, 0, None, 0, None) == pcx._lib.ERR_ARG
    assert L.pcx_fsync_process_dev(h, None, 5, None, 0, C.byref(r), None) == pcx._lib.ERR_ARG
    assert L.pcx_fsync_destroy(h) == 0


def test_block_is_registered_and_described():
    from pothoscomms_amd import blocks as B
    assert B.registry_arity("/comms/frame_sync", module="framesync") == 1 and B.registry_arity("/blocks/frame_sync", module="framesync") == 1
    text = open(SRC).read()
    assert "|PothosDoc Frame Sync" in text and "|alias /blocks/frame_sync" in text
    for key in ("outputMode", "preamble", "headerId", "symbolWidth", "dataWidth", "inputThreshold", "frameStartId", "frameEndId", "phaseOffsetID", "verboseMode"):
        assert re.search(r"\|param %s\b" % key, text) and re.search(r"\|setter set\w+\(%s\)" % key, text), key
    assert "|factory /comms/frame_sync(dtype)" in text


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_source_type_checks_against_the_pothos_surface():
    flags = ["-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-DPCX_WITH_POTHOS",
             "-I" + os.path.join(ROOT, "tests", "pothos_decl"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(SRC)]
    r = subprocess.run(["g++"] + flags + [SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def found_model(mode, dw, F, ids, off, first, dfc, poff, length):
    """FrameSync.cpp:537-586 in Python integers and doubles"""
    lw = 1 if mode == 2 else dw
    payload = off + first + 58 * dw + lw // 2
    l0, l1, remaining, phase = 0, (length - 1) * lw, length * dw, poff + dfc * float(F)
    if mode == 3:
        backup = min(payload, F)
        l0, l1, phase, remaining, payload = l0 + backup, l1 + backup, phase - dfc * float(backup), remaining + backup, payload - backup
    labels = []
    if ids[0]:
        labels.append((0, l0, lw, length, phase))
    if ids[1]:
        labels.append((1, l0, lw, length, 0.0))
    if ids[2]:
        labels.append((2, l1, lw, length, 0.0))
    return payload, remaining, phase, dfc, labels


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_side_alone_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "framesync_plan_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, os.path.join(ROOT, "tests", "framesync_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rng = np.random.default_rng(11)
    lines, want = [], []
    for k in range(600):            # seeded header words with no, one, two and three flipped bits, any word at all among them
        hid, length = int(rng.integers(0, 256)), int(rng.integers(0, 1 << 16))
        word = framer_model.header_word(hid, length) if k % 5 else int(rng.integers(0, 1 << 58))
        for b in rng.choice(58, size=k % 4, replace=False):
            word ^= 1 << int(b)
        expect = hid if k % 3 else 0x55
        bits = [(word >> i) & 1 for i in range(58)]
        did, dlen, dchk, bad = framer_model.header_decode(bits)
        ok = (not bad) and dchk == framer_model.header_checksum(did, dlen) and did == expect and dlen != 0
        lines.append("hdr %d %d" % (word, expect))
        want.append("%d %d %d %d %d" % (did, dlen, dchk, int(bad), int(ok)))
    found = []
    for k in range(400):
        mode, dw = int(rng.integers(0, 4)), int(rng.integers(2, 9))
        W = int(rng.integers(3, 30)) * dw * int(rng.integers(1, 6))
        F = W + 58 * dw
        off = int(rng.integers(-(W // 2) - 1, 5000))
        first = int(rng.integers(W // 2, F))
        ids = [int(v) for v in rng.integers(0, 2, 3)]
        dfc, poff, length = float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-np.pi, np.pi)), int(rng.integers(1, 4096))
        lines.append("found %d %d %d %d %d %d %d %d %r %r %d" % (mode, dw, F, ids[0], ids[1], ids[2], off, first, dfc, poff, length))
        found.append(found_model(mode, dw, F, ids, off, first, dfc, poff, length))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    got = run.stdout.splitlines()
    assert len(got) == len(lines) and got[:len(want)] == want
    for line, (payload, remaining, phase, inc, labels) in zip(got[len(want):], found):
        w = line.split()
        assert (int(w[0]), int(w[1]), float(w[2]), float(w[3]), int(w[4])) == (payload, remaining, phase, inc, len(labels)), line
        for k, (kind, index, width, length, value) in enumerate(labels):
            assert (int(w[5 + 5 * k]), int(w[6 + 5 * k]), int(w[7 + 5 * k]), int(w[8 + 5 * k]), float(w[9 + 5 * k])) == (kind, index, width, length, value), line
