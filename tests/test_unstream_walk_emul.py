"""The stream walk of LizardGPU_decompressStream_device / LizardGPU_streamIndex_device (lizard_amd/csrc/unstream_kernels.h: one wave
that follows the chain of frames across their boundaries) on the CPU SIMT emulator, under both lane schedules.  Streams are frames
made on the host (raw records assembled here, blocks of the oracle) joined back to back; the frame table must be what
LizardGPU_frameIndex answers when it is called frame by frame on the host, with each frame's offset, the control record must say
where and why the walk stopped, a launch must go on where the one before it stopped, entries behind the ones a launch wrote must
be left alone, and no byte outside src[0..srcSize) may be read."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_unframe_walk_emul as we

EMUL = we.EMUL
SEEDS = we.SEEDS
END, FULL, REFUSED = 1, 2, 3
E_GENERIC, E_RESERVED, E_HEADER_INCOMPLETE, E_FRAMETYPE = 1, 8, 12, 13


class Ctl(C.Structure):
    _fields_ = [("pos", C.c_uint64), ("nFrames", C.c_uint64), ("why", C.c_uint32), ("reserved", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libunstream_emul.so from simt.cpp + unstream_api.cpp, the way test_unframe_walk_emul.py builds its library."""
    out = os.path.join(EMUL, "libunstream_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "unstream_api.cpp")]
    deps = srcs + [os.path.join(EMUL, "lz_wave.h")] + [os.path.join(util.ROOT, "lizard_amd", "csrc", h) for h in ("unframe_walk.h", "unstream_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_unstream_walk.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint]
    L.emul_unstream_walk.restype = None
    return L


def test_the_control_record_is_the_one_the_host_file_reads():
    assert C.sizeof(Ctl) == 24 and C.sizeof(we.WalkResult) == 64


def host_table(stream):
    """What the loop over the host walk finds: ([(offset, rc, info, nRecords, frameBytes)], where it stopped, why)."""
    pos, out = 0, []
    while pos < len(stream):
        rc, info, _, _, n, fb = we.host(stream[pos:])
        out.append((pos, rc, info, n, fb))
        if rc:
            return out, pos, REFUSED
        pos += fb
    return out, pos, END


def walk(stream, table_cap, seed=1, start=0):
    """The stream walked from `start` the way the host drives the kernel: launches with a table of table_cap entries until one does
    not stop for a full table, each continuing from the control record the one before it left.
    ([(offset, WalkResult)], final control record, launches)."""
    L = lib()
    g = 64
    buf = (C.c_ubyte * (len(stream) + 2 * g))()
    C.memset(buf, 0x5A, len(buf))
    C.memmove(C.addressof(buf) + g, bytes(stream), len(stream))
    src = C.addressof(buf) + g
    ctl = Ctl()
    C.memset(C.byref(ctl), 0xEE, C.sizeof(ctl))
    ctl.pos = start
    entries, launches = [], 0
    while True:
        res, offs, span = (we.WalkResult * (table_cap + 2))(), (C.c_uint64 * (table_cap + 2))(), (C.c_longlong * 2)()
        C.memset(res, 0xEE, C.sizeof(res)); C.memset(offs, 0xEE, C.sizeof(offs))
        before = ctl.pos
        L.emul_unstream_walk(src, len(stream), C.byref(ctl), res, offs, table_cap, span, seed + launches)
        launches += 1
        assert 0 <= span[0] <= span[1] <= len(stream), ("the walk read outside the stream", list(span), len(stream))
        assert ctl.nFrames <= table_cap and ctl.why in (END, FULL, REFUSED) and ctl.reserved == 0 and before <= ctl.pos <= len(stream)
        k = ctl.nFrames
        assert bytes(res)[64 * k:] == b"\xEE" * (64 * (table_cap + 2 - k)) and bytes(offs)[8 * k:] == b"\xEE" * (8 * (table_cap + 2 - k)), \
            "an entry behind the ones this launch counted was written"
        for i in range(k):
            r = we.WalkResult.from_buffer_copy(bytes(res)[64 * i:64 * i + 64])
            entries.append((offs[i], r))
        if ctl.why == FULL:
            assert k == table_cap and ctl.pos < len(stream)
            continue
        return entries, ctl, launches


def check(stream, table_cap=64, name=""):
    """Both lane schedules against the host loop; returns the host table."""
    want, stop, why = host_table(stream)
    for seed in SEEDS:
        entries, ctl, launches = walk(stream, table_cap, seed)
        assert (ctl.pos, ctl.why) == (stop, why), (name, seed, ctl.pos, ctl.why, stop, why)
        assert len(entries) == len(want), (name, seed, len(entries), len(want))
        assert launches == max(1, -(-len(want) // table_cap)), (name, launches)
        for (off, r), (pos, rc, info, n, fb) in zip(entries, want):
            assert off == pos and -r.status == rc and r.done == 1, (name, seed, off, pos, r.status, rc)
            if rc:
                assert r.frameBytes == 0
                continue
            assert (r.nRecords, r.frameBytes, r.infoValid) == (n, fb, 1), (name, seed, pos)
            got = (0, 0, 0, 1, r.contentSize) if r.frameType else (r.blockSizeID, r.blockMode, r.checksumFlag, 0, r.contentSize)
            assert got == info, (name, seed, pos, got, info)
    return want, stop, why


@functools.lru_cache(maxsize=None)
def F():
    """Named host frames: raw-record frames of five block size ids with both header sizes and checksum on and off, an empty one, a
    skippable one, and the oracle-compressed frames of test_frame_index."""
    f = {"bs%d" % b: we.raw_frame([1000, 70 + b, 5], b, b & 1, (b >> 1) & 1, seed=20 + b) for b in (1, 2, 3, 4, 7)}
    f["records"] = we.raw_frame([131072, 1, 131072] + [33] * 130, 1, 1, 1, seed=4)          # more than two rounds of 64 records
    f["empty"] = we.raw_frame([], 1, 0, 0)
    f["empty checked"] = we.raw_frame([], 2, 1, 1)
    f["skip"] = we.SKIP
    f["checked"] = we.raw_frame([300, 40], 1, 1, 0, seed=9)
    f["sized"] = we.raw_frame([300, 40], 1, 0, 1, seed=10)
    for name, frame, _, _ in fi.frames_of_cases():
        f["oracle " + name] = frame
    return f


def test_one_frame():
    for name, frame in F().items():
        want, stop, why = check(frame, 4, name)
        assert len(want) == 1 and (stop, why) == (len(frame), END), name


def test_five_frames_of_mixed_block_size_ids():
    f = F()
    stream = b"".join(f["bs%d" % b] for b in (3, 1, 7, 2, 4))
    want, stop, why = check(stream, 8)
    assert [w[2][0] for w in want] == [3, 1, 7, 2, 4] and (stop, why) == (len(stream), END)
    oracle = [v for k, v in f.items() if k.startswith("oracle ")]
    assert len(oracle) >= 3
    want, stop, why = check(b"".join(oracle) + f["records"], 64)
    assert len(want) == len(oracle) + 1 and want[-1][3] == 133 and why == END


def test_empty_and_skippable_frames_between_others():
    f = F()
    for name, parts in (("an empty frame", ("bs1", "empty", "bs2")), ("empty frames alone", ("empty", "empty checked")),
                        ("a skippable frame in the middle", ("bs1", "sized", "skip", "checked", "bs3")), ("a skippable frame last", ("bs1", "skip"))):
        stream = b"".join(f[p] for p in parts)
        want, stop, why = check(stream, 16, name)
        assert len(want) == len(parts) and (stop, why) == (len(stream), END), name
        assert [w[2][3] for w in want] == [1 if p == "skip" else 0 for p in parts], name
        assert [w[3] for w in want] == [fi.index(f[p])[4] for p in parts], name


def test_a_table_of_three_entries_walked_in_segments_over_seven_frames():
    f = F()
    parts = ("bs1", "checked", "skip", "bs4", "empty", "sized", "bs7")
    stream = b"".join(f[p] for p in parts)
    want, stop, why = check(stream, 3)
    assert len(want) == 7 and why == END
    for seed in SEEDS:
        entries, ctl, launches = walk(stream, 3, seed)
        assert launches == 3 and [e[0] for e in entries] == [w[0] for w in want]
        # a launch starts where its control record says: from the fourth frame on
        tail, ctl, launches = walk(stream, 3, seed, start=want[3][0])
        assert [e[0] for e in tail] == [w[0] for w in want[3:]] and launches == 2 and ctl.why == END
        # six frames and a table of three: the second launch fills the table as the stream ends, and says so
        six = stream[:want[6][0]]
        entries, ctl, launches = walk(six, 3, seed)
        assert len(entries) == 6 and (ctl.pos, ctl.why, launches) == (len(six), END, 2)
    # a table of one entry: a launch per frame
    assert walk(stream, 1)[2] == 7


def damaged_streams():
    """(name, stream, frames in front of the refused one, its status)."""
    f = F()
    head = f["bs1"] + f["checked"]
    out = []
    for name, frame in (("bs2", f["bs2"]), ("sized", f["sized"])):
        for cut in sorted({1, 3, 4, 6, len(frame) > 30 and 14 or 6}):
            out.append(("cut inside the header of %s at %d" % (name, cut), head + frame[:cut], 2, E_HEADER_INCOMPLETE))
    rec = f["records"]
    out.append(("cut inside a record", head + rec[:15 + 4 + 1000], 2, E_GENERIC))
    out.append(("cut inside a record word", head + rec[:15 + 2], 2, E_GENERIC))
    out.append(("cut before the end mark", head + f["bs1"][:-4], 2, E_GENERIC))
    out.append(("cut before a checksum", head + f["checked"][:-4], 2, E_GENERIC))
    out.append(("cut inside a checksum", head + f["checked"][:-1], 2, E_GENERIC))
    out.append(("cut inside a skippable frame", head + f["skip"][:-1], 2, E_GENERIC))
    out.append(("4 bytes of garbage behind frame 2", head + b"\xde\xad\xbe\xef" + f["bs3"], 2, E_FRAMETYPE))
    out.append(("4 bytes of garbage at the end", head + b"\xde\xad\xbe\xef", 2, E_HEADER_INCOMPLETE))
    bad = bytearray(f["bs3"]); bad[4] |= 2
    out.append(("a reserved header bit set in frame 3", head + bytes(bad) + f["bs4"], 2, E_RESERVED))
    bad = bytearray(f["sized"]); bad[5] |= 0x80
    out.append(("a reserved bit of the second header byte set in frame 3", head + bytes(bad) + f["bs4"], 2, E_RESERVED))
    out.append(("the first frame refused", b"\xde\xad\xbe\xef" + head, 0, E_FRAMETYPE))
    return out


@pytest.mark.parametrize("case", damaged_streams(), ids=lambda c: c[0])
def test_the_walk_stops_at_the_frame_the_host_walk_refuses(case):
    name, stream, ahead, status = case
    f = F()
    for cap in (64, 2):
        want, stop, why = check(stream, cap, name)
        assert why == REFUSED and len(want) == ahead + 1 and want[-1][1] == -status, (name, want[-1][1], status)
        assert stop == want[-1][0] == (len(f["bs1"] + f["checked"]) if ahead else 0), name
    # the table is full with the frame in front of the refused one: the refusal is the next launch's only entry
    if ahead:
        entries, ctl, launches = walk(stream, ahead)
        assert launches == 2 and len(entries) == ahead + 1 and ctl.nFrames == 1 and ctl.why == REFUSED and entries[-1][1].status == status
