"""CPU: the inputs of tests/count_trip_inputs.py through the producer / consumer form of levels 10 / 30 on the SIMT emulator
(tests/emul/count_trip_api.cpp: as on the device, the level-10 producers run the lane forms — the late back trip of lz_block.h — and the
level-30 producers the two count calls in a row), byte for byte against the oracle, with the switch off and on.  The marks (lz_block.h, LZ_CT_MARK) must show for every input the trips that the serial model of
count_trip_inputs.parse predicts from its sequences — so each input took the path it was built for — and the model itself is held
to the oracle's stream sizes on every block.  The stand-alone program tests/count_trip_asan_main.cpp runs the same blocks under
AddressSanitizer with sources of exactly n bytes."""
import os
import re
import struct
import subprocess

import pytest

import count_trip_emul as emul
import count_trip_inputs as inputs
import util

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = (1, 0)                                    # LZ_BACK_LATE


@pytest.fixture(scope="module")
def libs():
    out = {sw: emul.lib(late=sw) for sw in SWITCHES}
    for sw, L in out.items():
        assert emul.knobs(L)[0] == sw
    assert emul.knobs(emul.lib())[0] == 1, "the tree builds the level-10 producers without the late back trip"
    return out


def _one(L, data, level, seed=1, **kw):
    return emul.run(L, data, [(0, len(data))], level, seed=seed, **kw)[0]


def test_every_input_holds_its_case():
    """The matrix of the module's text is complete, every block has the size asked for, and the oracle alone gives the sequences the
    model gives."""
    got = {name: s for name, _, s in inputs.cases()}
    for L in inputs.FWD:
        s = got["fwd%d" % L]
        assert s["fwd"] == L and s["back"] == 0 and s["fwd_open"] == (L >= 24) and not s["back_open"]
    for b in inputs.BACK:
        s = got["back%d" % b]
        assert s["back"] == b and s["room"] > b and not s["fwd_open"] and s["back_open"] == (b >= 8)
    for f in inputs.BOTH_FWD:
        for b in inputs.BOTH_BACK:
            s = got["both_f%d_b%d" % (f, b)]
            assert (s["fwd"], s["back"]) == (f, b) and s["fwd_open"] and s["back_open"]
    s = got["to_matchlimit"]
    assert s["P"] + s["fwd"] == s["matchlimit"] and s["fwd_open"] and s["back_open"]
    s = got["beyond_mflimit"]
    assert s["mflimit"] < s["P"] + s["fwd"] < s["matchlimit"] and s["fwd_open"] and s["back_open"]
    for d in (3, 7):
        s = got["block_start_p%d" % d]
        assert s["back"] == s["M"] > 8                                   # cut by the candidate's distance from the block start
    s = got["sweep_inside"]
    assert s["P"] < 32768 < s["P"] + s["fwd"] and s["fwd_open"] and s["back_open"]
    for f in (12, 40):
        s = got["anchor_cut9_f%d" % f]
        assert (s["back"], s["room"], s["fwd"]) == (9, 9, f) and s["back_open"] and s["fwd_open"] == (f >= 24)
    far = {name: (data, s) for name, data, s in inputs.far_cases()}
    for cut in inputs.ANCHOR_FAR:                                        # cut by the anchor, the bytes go on: back alone and both open
        for f in (12, 32):
            data, s = far["anchor_cut%d_f%d" % (cut, f)]
            assert (s["back"], s["room"], s["fwd"]) == (cut, cut, f) and s["back_open"] and s["fwd_open"] == (f >= 24)
            assert data[s["P"] - cut - 1] == data[s["M"] - cut - 1] and len(data) < 70000
    start = {name: s for name, _, s in inputs.start_cases()}
    for M in inputs.START_M:                                             # cut by the block start at 63, 64, 65: back alone and both open
        for f in (12, 32):
            s = start["start_cut%d_f%d" % (M, f)]
            assert s["M"] == M == s["back"] and s["room"] > M and s["back_open"] and s["fwd"] == f and s["fwd_open"] == (f >= 24)
    # (anchor cuts of 0 .. 8 bytes with a room of 0, 1, 7, 8, 9, and candidates 0 .. 9 bytes from the block start: producer_latch_inputs,
    #  whose own test holds that matrix complete)
    assert len(inputs.anchor_cases()) == len(inputs.latch.back_blocks()) + len(inputs.latch.low_blocks())
    for name, data, _ in inputs.cases() + inputs.far_cases() + inputs.start_cases():
        assert inputs.model_exact(data), name
        assert 1900 <= len(data) <= 16384 or name == "sweep_inside" or name.startswith("anchor_cut"), (name, len(data))
    name, data, s = inputs.second_subblock()
    assert len(data) == 131072 + 9000 and s["sub"] == 1 and s["fwd_open"] and s["back_open"]
    for level in inputs.LEVELS:
        assert None not in inputs.stream_sizes(inputs.expected(level)[name])


@pytest.mark.parametrize("switches", SWITCHES)
@pytest.mark.parametrize("level", inputs.LEVELS)
def test_every_input_byte_for_byte(libs, level, switches):
    want = inputs.expected(level)
    for case, (name, data) in enumerate(inputs.all_blocks()):
        assert _one(libs[switches], data, level, seed=case + 1) == want[name], (level, switches, name)


@pytest.mark.parametrize("switches", SWITCHES)
def test_lane_forms_at_level_30_too(libs, switches):
    """The level-10 producer in front of the level-30 consumer (the emulator's other libraries run it so): the new trips do not depend
    on what consumes the sequences."""
    want = inputs.expected(30)
    for case, (name, data, _) in enumerate(inputs.cases()):
        assert _one(libs[switches], data, 30, seed=case + 3, lane_forms=1) == want[name], (switches, name)


@pytest.mark.parametrize("switches", SWITCHES)
def test_paths_are_taken(libs, switches):
    """Level 10.  Marks: 3 late back trips, 8 forward trips, 9 back trips in the parent's place.  A winner with both lengths open takes
    its forward trip where it stood and its back trip late; with the switch off the back trips are taken the parent's way, and
    nothing else moves."""
    late = switches
    L = libs[switches]
    blocks = [(n, d) for n, d, _ in inputs.cases() + inputs.far_cases() + inputs.start_cases()] + [inputs.second_subblock()[:2]]
    blocks += list(inputs.anchor_cases()[:10])
    seen = {k: 0 for k in (3, 8, 9)}
    for name, data in blocks:
        m = inputs.marks_of(inputs.parse(data))
        want = {3: m["back"] if late else 0, 8: m["fwd"], 9: 0 if late else m["back"]}
        emul.marks(L)
        assert _one(L, data, 10) == inputs.expected(10)[name], (switches, name)
        got = emul.marks(L)
        assert {k: got[k] for k in want} == want, (switches, name, got, want)
        for k in seen:
            seen[k] += got[k]
    assert (seen[3] > 0) == bool(late) and (seen[9] > 0) == (not late) and seen[8] > 0


def test_two_producers_share_the_inputs(libs):
    """The one-sub-block inputs as one ragged batch at odd addresses over two producers: nothing of a block's trips stays behind for
    the next block of the same producer."""
    blocks, area = [], bytearray()
    for name, data, _ in inputs.cases():
        area += b"\x5a" * (2 - len(area) % 2)                           # (every block starts at an odd offset)
        blocks.append((len(area), len(data)))
        area += data
    for level in inputs.LEVELS:
        outs = emul.run(libs[1], bytes(area), blocks, level, nprod=2, ncons=1, seed=9)
        for (name, data, _), out in zip(inputs.cases(), outs):
            assert out == inputs.expected(level)[name], (level, name)


def test_same_blocks_under_address_sanitizer(tmp_path):
    """tests/count_trip_asan_main.cpp as a program of its own: every block in an allocation of exactly its size, levels 10 and 30; exit
    status 0, no report, every output the oracle's.  A toolchain without the sanitizers' runtime fails this test."""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    cxx = ["-std=c++17", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread"]
    blocks = inputs.all_blocks()
    path = tmp_path / "blocks.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blocks)))
        for _, data in blocks:
            f.write(struct.pack("<I", len(data)) + data)
    api = os.path.join(emul.EMUL, "count_trip_api.cpp")
    jobs = [(["gcc", "-std=gnu99"], os.path.join(util.ORACLE_DIR, "lizard_oracle.c"), "oracle.o"),
            (["gcc", "-std=gnu99"], os.path.join(util.ORACLE_DIR, "huf_oracle.c"), "huf.o"),
            (["g++"] + cxx + ["-I", emul.EMUL], os.path.join(emul.EMUL, "simt.cpp"), "simt.o"),
            (["g++"] + cxx + ["-I", emul.EMUL], api, "api_default.o"),
            (["g++"] + cxx, os.path.join(HERE, "count_trip_asan_main.cpp"), "main.o")]
    procs = []
    for cmd, src, obj in jobs:
        procs.append(subprocess.Popen(cmd + san + ["-c", src, "-o", str(tmp_path / obj)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        log = p.communicate()[0]
        assert p.returncode == 0, "the sanitized program does not build:\n" + log[-3000:]
    for api_obj in ("api_default.o",):
        exe = str(tmp_path / ("count_trip_asan_" + api_obj[4:-2]))
        objs = [str(tmp_path / o) for o in ("oracle.o", "huf.o", "simt.o", api_obj, "main.o")]
        subprocess.run(["g++"] + san + ["-pthread"] + objs + ["-o", exe], check=True, capture_output=True, text=True)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        tail = (r.stdout + r.stderr)[-4000:]
        assert r.returncode == 0, tail
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
        m = re.fullmatch(r"cases: (\d+) mismatches: (\d+) late: (\d+)", r.stdout.strip().splitlines()[-1])
        assert m and int(m.group(2)) == 0 and int(m.group(3)) > 0, tail
        assert int(m.group(1)) == 2 * len(blocks), tail
