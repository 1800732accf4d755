"""The frame walk of LizardGPU_decompressFrame_device / LizardGPU_frameIndex_device (lizard_amd/csrc/unframe_walk.h) on the CPU
SIMT emulator, under both lane schedules, against the host walk LizardGPU_frameIndex: intact frames of every shape, any
segmentation, and damaged frames — the same return code in every case, and no byte read outside src[0..srcSize)."""
import collections
import ctypes as C
import functools
import os
import random
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_frame_decompress_gpu as fd

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
SEEDS = (1, 0x9E3779B9)
ALL = 1 << 62


class WalkResult(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("status", "done", "infoValid", "frameType", "blockSizeID", "blockMode", "checksumFlag", "headerBytes")] \
             + [(n, C.c_uint64) for n in ("contentSize", "nRecords", "nextPos", "frameBytes")]


@functools.lru_cache(maxsize=None)
def walk_lib():
    """tests/emul/libunframe_walk_emul.so from simt.cpp + unframe_walk_api.cpp, the way test_unframe_emul.py builds its library."""
    out = os.path.join(EMUL, "libunframe_walk_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "unframe_walk_api.cpp")]
    deps = srcs + [os.path.join(EMUL, "lz_wave.h"), os.path.join(util.ROOT, "lizard_amd", "csrc", "unframe_walk.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_unframe_walk.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.emul_unframe_walk.restype = None
    return L


def walk(frame, budget=ALL, seed=1, table_cap=None):
    """The walk in segments of `budget` records, driven the way the host drives the kernel:
    (rc, info fields, offsets, words, nRecords, frameBytes, segments).  Asserts that every read stayed inside the frame."""
    L = walk_lib()
    g = 64
    buf = (C.c_ubyte * (len(frame) + 2 * g))()
    C.memset(buf, 0x5A, len(buf))
    C.memmove(C.addressof(buf) + g, bytes(frame), len(frame))
    src = C.addressof(buf) + g
    pos, offs, words, info, segs, total = 0, [], [], (0, 0, 0, 0, 0), 0, 0
    while True:
        res, span = WalkResult(), (C.c_longlong * 2)()
        cap = min(budget, 1 << 16) if table_cap is None else table_cap
        o, w = (C.c_uint64 * max(cap, 1))(), (C.c_uint32 * max(cap, 1))()
        L.emul_unframe_walk(src, len(frame), pos, budget, cap, o, w, C.byref(res), span, seed)
        segs += 1
        assert 0 <= span[0] <= span[1] <= len(frame), ("the walk read outside the frame", list(span), len(frame))
        if segs == 1 and res.infoValid:
            info = (0, 0, 0, 1, res.contentSize) if res.frameType else (res.blockSizeID, res.blockMode, res.checksumFlag, 0, res.contentSize)
        if res.status:
            assert res.done == 1
            return -res.status, info, [], [], 0, 0, segs
        assert res.nRecords <= budget
        k = min(res.nRecords, cap)
        offs += list(o)[:k]; words += list(w)[:k]; total += res.nRecords
        if res.done:
            return 0, info, offs, words, total, res.frameBytes, segs
        assert res.nRecords == budget and res.nextPos > pos
        pos = res.nextPos


def host(frame):
    rc, info, offs, words, n, fb = fi.index(frame)
    return rc, (info.blockSizeID, info.blockMode, info.contentChecksumFlag, info.frameType, info.contentSize), offs, words, n, fb


def raw_frame(pieces, bsid=1, checksum=0, csize=0, seed=3):
    """A frame assembled here from stored-raw records of the given sizes."""
    import xxhash
    rnd = random.Random(seed)
    data = [rnd.randbytes(n) for n in pieces]
    total = sum(pieces)
    hdr = bytes([(1 << 6) | (1 << 5) | (checksum << 2) | (csize << 3), bsid << 4]) + (struct.pack("<Q", total) if csize else b"")
    out = struct.pack("<I", 0x184D2206) + hdr + bytes([(xxhash.xxh32(hdr, seed=0).intdigest() >> 8) & 255])
    for d in data:
        out += struct.pack("<I", len(d) | 0x80000000) + d
    out += struct.pack("<I", 0)
    if checksum:
        out += struct.pack("<I", xxhash.xxh32(b"".join(data), seed=0).intdigest())
    return out


SKIP = struct.pack("<II", 0x184D2A57, 9) + b"skippable"


@functools.lru_cache(maxsize=None)
def intact():
    """(name, frame): the frame cases (block compressor: the oracle, no GPU), the committed reference frames, frames of raw
    records with 7- and 15-byte headers with and without checksum, a skippable frame, empty frames."""
    out = [(name, frame) for name, frame, _, _ in fi.frames_of_cases()]
    out += [(name, frame) for name, frame, _, _ in fd.reference_frames()]
    for checksum in (0, 1):
        for csize in (0, 1):
            out.append(("raw c%d s%d" % (checksum, csize), raw_frame([131072, 1, 70, 131072, 4097, 5, 66, 1000] + [33] * 130, 1, checksum, csize)))
            out.append(("empty c%d s%d" % (checksum, csize), raw_frame([], 2, checksum, csize)))
    out.append(("raw bs256k", raw_frame([262144, 262144, 9], 2, 1, 0)))
    out.append(("skippable", SKIP))
    out.append(("skippable empty", struct.pack("<II", 0x184D2A50, 0)))
    return out


def test_intact_frames_match_the_host_walk():
    shapes = set()
    for name, frame in intact():
        want = host(frame)
        assert want[0] == 0, name
        for seed in SEEDS:
            assert walk(frame, seed=seed)[:6] == want, (name, seed)
        assert walk(frame + b"\x04\x22\x4d\x18tail")[:6] == want, name       # the walk ends where the frame ends
        shapes.add((len(frame) > 8 and frame[4] & 8, want[1][2], want[1][3]))
    assert len(shapes) >= 5, shapes                                           # both header sizes x checksum, and skippable
    # a short table is filled as far as it goes and the count is still the frame's
    name, frame = intact()[3]
    want = host(frame)
    assert want[4] > 1
    got = walk(frame, table_cap=1)
    assert (got[0], got[2], got[3], got[4], got[5]) == (0, want[2][:1], want[3][:1], want[4], want[5])


def test_concatenated_frames_are_walked_one_after_the_other():
    frames = [f for _, f in intact()]
    rnd = random.Random(11)
    stream = b"".join(frames)
    pos = 0
    for f in frames:
        rc, info, offs, words, n, fb, _ = walk(stream[pos:pos + len(f) + 5000], budget=rnd.choice((1, 7, ALL)), seed=rnd.choice(SEEDS))
        assert (rc, info, offs, words, n, fb) == host(f)
        pos += fb
    assert pos == len(stream)


def test_any_segmentation_gives_the_same_table():
    for name, frame in intact():
        want = host(frame)
        for budget in (1, 2, 3, ALL):
            for seed in SEEDS:
                got = walk(frame, budget, seed)
                assert got[:6] == want, (name, budget, seed)
                if want[1][3] == 0:
                    assert got[6] == (1 if budget == ALL else want[4] // budget + 1), (name, budget)


def damaged_cases():
    """(name, damaged frame): damage() over the intact frames, and every truncation of two short frames."""
    rnd = random.Random(20261017)
    out = []
    bases = [(n, f) for n, f in intact() if len(f) > 8]
    for name, frame in bases:
        for _ in range(1800 // len(bases) + 1):
            kind, bad = fd.damage(rnd, frame)
            out.append((name + " " + kind, bad))
    for name, frame in (("raw", raw_frame([70, 1, 33], 1, 1, 1)), ("skippable", SKIP)):
        out += [("%s cut %d" % (name, cut), frame[:cut]) for cut in range(len(frame))]
    short = raw_frame([5, 40], 1, 1, 0)
    for at in range(len(short)):
        for bit in (0, 7):
            out.append(("short flip %d.%d" % (at, bit), short[:at] + bytes([short[at] ^ (1 << bit)]) + short[at + 1:]))
    return out


def test_damaged_frames_get_the_host_walk_s_answer():
    cases = damaged_cases()
    counts = collections.Counter()
    rnd = random.Random(5)
    for name, bad in cases:
        want = host(bad)
        for seed in SEEDS:
            got = walk(bad, rnd.choice((1, 2, 3, ALL)), seed)
            assert got[0] == want[0], (name, got[0], want[0])
            assert got[:6] == want, name
        counts["accepted" if want[0] == 0 else "refused %d" % -want[0]] += 1
    total = len(cases)
    refused = total - counts["accepted"]
    print("%d damaged frames: %s" % (total, dict(counts)))
    assert total >= 2000
    assert counts["accepted"] > total // 20 and refused > total // 20, counts
    assert {k for k in counts if k != "accepted"} >= {"refused %d" % e for e in (1, 2, 6, 7, 8, 12, 13, 17)}, counts
