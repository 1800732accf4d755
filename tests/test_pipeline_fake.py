"""CPU: the two host pipelines — LizardGPU_decompressFrame (lizard_amd/csrc/lizard_unframe_host.c) and run_host_job with its drain
thread (lizard_pipeline_host.c) — on a fake HIP runtime whose streams DEFER their work (tests/fake_hip.c, tests/pipeline_fake.c).
A copy or a "kernel" reads its arguments when the fake decides to run it: eagerly, as late as the host's waits allow, or in a
seeded random interleaving.  A missing event wait, a staging buffer reused too early or a result read too early is wrong bytes
here on every run, not a timing accident.  The kernels are the real bodies on the SIMT emulator (lz_unframe_record, the block
decoder) and the oracle; results are compared with the plain bytes, the oracle and the host decoder LizardF_decompress.

Wall time of this module, measured on the CPU box: 105 s (28 tests; 34 s of it are the two sanitizer programs) against 532 s for the
rest of the CPU suite: below the quarter the module may take.  The emulated decoder does about 5 MB/s, which sizes the cases:
frames of 0.3 - 1.3 MiB, 128 KiB blocks, chunks of 256 KiB (2 records) and 1 MiB (8 records)."""
import atexit
import collections
import ctypes as C
import functools
import os
import random
import shutil
import struct
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_frame_decompress_gpu as tg
from golden.make_frame_golden import golden_frame_input

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(util.ROOT, "lizard_amd", "csrc")
EAGER, LAZY, RANDOM = 0, 1, 2
SCHEDULES = [("eager", EAGER, 1), ("lazy", LAZY, 1), ("random", RANDOM, 101), ("random", RANDOM, 202), ("random", RANDOM, 303)]
E_GENERIC, E_TOO_SMALL, E_FAILED = 1, 11, 16
CANARY = 0xC3
KIB = 1024
_dir = tempfile.mkdtemp(prefix="pipeline_fake_")
atexit.register(shutil.rmtree, _dir, True)


@functools.lru_cache(maxsize=None)
def built(kind):
    """'lib': the harness as a shared library for ctypes; 'asan' / 'tsan': as a program with that sanitizer.  The emulator's objects
    are built plain in every form (its lanes switch stacks by hand, which the sanitizers' instrumentation does not follow).
    lizard_unframe_device.c (tests/test_pipeline_fake_device.py) is compiled in with a small odd piece size for its checksum pass."""
    return util.build_fake(_dir, kind, "pipeline_fake", ("pipeline_fake.c", "fake_hip.c"))


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built("lib"))
    H.fh_set_abort(0)                                       # a failed check of the fake is collected by ok() instead of killing pytest
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.fh_register_pinned.argtypes = [C.c_void_p, C.c_size_t]
    H.fh_unregister_pinned.argtypes = [C.c_void_p]
    H.fh_ops_run.restype = C.c_ulonglong
    H.pf_set_chunk_bytes.argtypes = [C.c_size_t]
    H.LizardGPU_decompressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    H.LizardGPU_decompressFrame.restype = C.c_size_t
    H.LizardGPU_frameDecodePackedChunks.restype = C.c_ulonglong
    H.LizardGPU_lastError.restype = C.c_char_p
    H.LizardF_isError.argtypes = [C.c_size_t]; H.LizardF_isError.restype = C.c_uint
    H.LizardGPU_compressBlocks_host.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    H.LizardGPU_compressBlocks_host_packed.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
    H.LizardGPU_decompressBlocks_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    H.Lizard_decompress_safe_usingDict.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    H.LizardF_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]; H.LizardF_compressFrame.restype = C.c_size_t
    H.LizardF_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]; H.LizardF_compressFrameBound.restype = C.c_size_t
    for name in ("LizardF_compressBegin", "LizardF_compressEnd", "LizardF_flush", "LizardF_compressUpdate", "LizardF_createCompressionContext"):
        getattr(H, name).restype = C.c_size_t
    H.LizardF_compressBegin.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    H.LizardF_compressUpdate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p]
    H.LizardF_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    H.LizardF_compressEnd.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    H.LizardF_createCompressionContext.argtypes = [C.c_void_p, C.c_uint]
    H.LizardF_freeCompressionContext.argtypes = [C.c_void_p]
    return H


def ok(what=""):
    """No check of the fake runtime failed since the last look (bounds, pinned host sides, queues empty at lzk_guard_release)."""
    buf = C.create_string_buffer(512)
    n = harness().fh_violations(buf, 512)
    assert n == 0, (what, n, buf.value)


def schedule(s, chunk=256 * KIB):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    H.pf_set_chunk_bytes(chunk)


def err_of(r):
    return (1 << 64) - r if harness().LizardF_isError(r) else 0


def stats():
    out = (C.c_ulonglong * 4)()
    assert harness().LizardGPU_frameDecodeStats(out) == 0
    return list(out)


def decode(frame, cap, pinned=False):
    """(error number or 0, consumed, bytes): canaries around dst; a pinned source is registered memory, the frame at an odd offset."""
    H = harness()
    g = 4096
    src = (C.c_ubyte * (len(frame) + 64))()
    C.memset(src, 0x5A, len(src))
    at = C.addressof(src) + (3 if pinned else 16)
    C.memmove(at, bytes(frame), len(frame))
    out = (C.c_ubyte * (cap + 2 * g))()
    C.memset(out, CANARY, len(out))
    used = C.c_size_t(12345)
    if pinned:
        H.fh_register_pinned(src, len(src))
    r = H.LizardGPU_decompressFrame(C.addressof(out) + g, cap, at, len(frame), C.byref(used))
    if pinned:
        H.fh_unregister_pinned(src)
    raw = bytes(out)
    assert raw[:g] == bytes([CANARY]) * g and raw[g + cap:] == bytes([CANARY]) * g, "the frame decoder wrote outside dst"
    e = err_of(r)
    if e:
        assert used.value == 0
        return e, 0, b""
    assert r <= cap
    return 0, used.value, raw[g:g + r]


def check_frame(frame, plain, what, s, host=True, light=True):
    """Both kinds of source; capacities exact, the bound and exact - 1; the host decoder in one call.  light: the capacities are
    shared out between the two kinds of source instead of all running with both (the emulated decoder does 5 MB/s)."""
    b = fi.bound(frame)
    assert not fi.err_of(b) and b >= len(plain), what
    for pinned in (False, True):
        for cap in ((b,) if pinned else (len(plain),)) if light else (len(plain), b if pinned else len(plain) + 77):
            e, used, got = decode(frame, cap, pinned)
            assert (e, used) == (0, len(frame)), (what, s, pinned, cap, e, harness().LizardGPU_lastError())
            assert got == plain, (what, s, pinned, cap)
        if len(plain) and not (light and pinned):
            assert decode(frame, len(plain) - 1, pinned)[0] == E_TOO_SMALL, (what, s, pinned)
        ok((what, s, pinned))
    if host:
        he, hint, hused, hgot = fi.host_one_call(frame, len(plain) + 16)
        assert (he, hint, hused) == (0, 0, len(frame)) and hgot == plain, what


def fake_frame(data, level=10, bsid=1, checksum=1, csize=0, mode=1):
    """LizardF_compressFrame inside the fake: the records come out of lzgpu_frame_records on the deferred streams."""
    H = harness()
    p = util.frame_prefs(level, bsid, checksum, len(data) if csize else 0, mode)
    cap = H.LizardF_compressFrameBound(len(data), C.byref(p))
    dst = C.create_string_buffer(cap)
    n = H.LizardF_compressFrame(dst, cap, bytes(data), len(data), C.byref(p))
    assert not err_of(n), err_of(n)
    ok("LizardF_compressFrame")
    return dst.raw[:n]


def fake_flushed(data, pieces, level=10, bsid=1, mode=1, checksum=1):
    """compressUpdate + flush after every piece, inside the fake: short records in the middle of the frame."""
    H = harness()
    ctx = C.c_void_p()
    assert H.LizardF_createCompressionContext(C.byref(ctx), 100) == 0
    p = util.frame_prefs(level, bsid, checksum, 0, mode)
    cap = H.LizardF_compressFrameBound(len(data), C.byref(p)) + (len(pieces) + 2) * (util.FRAME_BLOCK_SIZES[bsid] + 64)
    dst = C.create_string_buffer(cap)
    pos = H.LizardF_compressBegin(ctx, dst, cap, C.byref(p))
    assert not err_of(pos)
    at = 0
    for n in pieces:
        for fn, args in ((H.LizardF_compressUpdate, (bytes(data[at:at + n]), n, None)), (H.LizardF_flush, (None,))):
            r = fn(ctx, C.addressof(dst) + pos, cap - pos, *args)
            assert not err_of(r)
            pos += r
        at += n
    assert at == len(data)
    r = H.LizardF_compressEnd(ctx, C.addressof(dst) + pos, cap - pos, None)
    assert not err_of(r)
    H.LizardF_freeCompressionContext(ctx)
    ok("flushed frame")
    return dst.raw[:pos + r]


@functools.lru_cache(maxsize=None)
def inputs():
    d = util.datagen(5 * 131072 + 4321, 0.5, 0.0, 97)
    return {"p50": d, "text": (b"the quick brown fox jumps over the lazy dog. " * 9000)[:3 * 131072 - 17], "noise": random.Random(3).randbytes(300000)}


def golden(name):
    return open(os.path.join(util.GOLDEN_DIR, name), "rb").read()


# ---------------------------------------------------------------- whole frames ------------------------------------------------

@pytest.mark.parametrize("s", SCHEDULES, ids=lambda s: "%s%d" % (s[0], s[2]))
def test_whole_frames(s):
    H = harness()
    d = inputs()
    schedule(s, 1024 * KIB if s[2] == 202 else 256 * KIB)
    if s[1] == LAZY:
        H.pf_shutdown()                                     # fresh (poisoned) staging under the schedule that runs everything as late as it may
    # composed from oracle blocks
    s0 = stats()
    check_frame(util.compose_frame(d["p50"], 10, 1, 1, 0, util.oracle_compress), d["p50"], "composed L10", s)
    check_frame(util.compose_frame(d["text"], 30, 1, 0, 1, util.oracle_compress), d["text"], "composed L30", s)
    s1 = stats()
    assert s1[2:] == s0[2:] and s1[0] > s0[0], "a frame of independent blocks reached the host decoder"
    # written inside the fake: LizardF_compressFrame (independent: byte-equal to the restatement on the oracle), linked
    f = fake_frame(d["p50"], 10, 1, 1, 1, 1)
    assert f == util.compose_frame(d["p50"], 10, 1, 1, 1, util.oracle_compress)
    check_frame(f, d["p50"], "fake independent", s, light=False)
    check_frame(fake_frame(d["text"], 21, 1, 1, 0, 0), d["text"], "fake linked", s)
    assert stats()[2:] == s0[2:], "a frame of this library reached the host decoder"
    # all raw; a raw record shorter than the block size in the middle
    f_raw = fake_frame(d["noise"], 10, 1, 1, 0, 1)
    assert all(w >> 31 for w in fi.index(f_raw)[3])
    c0 = stats()[0]
    check_frame(f_raw, d["noise"], "all raw", s)
    assert stats()[0] == c0
    before = H.LizardGPU_frameDecodePackedChunks()
    f = fake_flushed(d["noise"], [100000, 131072, 68928], checksum=0)
    assert all(w >> 31 for w in fi.index(f)[3])
    check_frame(f, d["noise"], "raw flushed", s)
    # short compressed records in the middle: the packed path
    pieces = [131072, 1, 70000, 131073, 5, len(d["p50"]) - (131072 + 1 + 70000 + 131073 + 5)]
    for mode in (1, 0):
        f = fake_flushed(d["p50"], pieces, mode=mode)
        assert fi.index(f)[4] > len(pieces)
        check_frame(f, d["p50"], ("flushed", mode), s, light=bool(mode))
    assert H.LizardGPU_frameDecodePackedChunks() > before, "the compaction path did not run"
    # degenerate frames and a concatenation
    one = fake_frame(b"x", 10, 1, 1, 0, 1)
    check_frame(one, b"x", "one byte", s)
    for checksum in (0, 1):
        empty = fake_frame(b"", 10, 1, checksum, 0, 1)
        assert decode(empty, 0) == (0, len(empty), b"") and decode(empty, 100, True) == (0, len(empty), b"")
    skip = struct.pack("<II", 0x184D2A57, 9) + b"skippable"
    assert decode(skip, 0) == (0, len(skip), b"") and decode(skip + b"tail", 5, True) == (0, len(skip), b"")
    small = d["text"][:70000]
    stream = skip + fake_frame(small, 21, 1, 1, 1, 1) + one + skip + f_raw
    pos, out = 0, []
    while pos < len(stream):
        e, used, got = decode(stream[pos:], 1 << 20, pinned=bool(len(out) & 1))
        assert e == 0 and used > 0
        out.append(got)
        pos += used
    assert out == [b"", small, b"x", b"", d["noise"]] and pos == len(stream)
    ok(s)


@pytest.mark.parametrize("s", SCHEDULES, ids=lambda s: "%s%d" % (s[0], s[2]))
def test_reference_frames_and_the_give_up_threshold(s):
    """The committed reference-made frames (and fresh ones where oracle/_ref is present).  Records of the linked frame need their
    history; LIZARDGPU_UNFRAME_HOST_SHARE = 2 (never give up) and 0 (after the first chunk) give the same bytes."""
    plain = golden_frame_input()
    schedule(s)
    frames = [("golden linked", golden("frame_ref_linked.liz"), plain, True), ("golden independent", golden("frame_ref_independent.liz"), plain, False)]
    if util.reference() is not None and s[2] in (1, 101):
        data = inputs()["p50"]
        for mode in (0, 1):
            frames.append(("fresh reference %d" % mode, util.reference_frame(data, util.frame_prefs(17, 1, 1, len(data), mode)), data, mode == 0))
    for name, frame, data, linked in frames:
        s0 = stats()
        check_frame(frame, data, name, s)
        s1 = stats()
        if linked:
            assert s1[2] > s0[2], "no block of the reference's linked frame needed its history"
        else:
            assert s1[2:] == s0[2:] and sum(s1[:2]) - sum(s0[:2]) >= 2 * fi.index(frame)[4]
    name, frame, data, _ = frames[0]
    seen = {}
    try:
        for share in ("2", "0"):
            os.environ["LIZARDGPU_UNFRAME_HOST_SHARE"] = share
            s0 = stats()
            for pinned in (False, True):
                assert decode(frame, len(data), pinned) == (0, len(frame), data), (share, s)
            s1 = stats()
            seen[share] = (s1[2] - s0[2], s1[3] - s0[3])
            ok((share, s))                                  # the hand-over leaves chunks in flight: they are drained before the context is released
    finally:
        del os.environ["LIZARDGPU_UNFRAME_HOST_SHARE"]
    assert seen["2"][1] == 0 and seen["2"][0] >= 4, seen
    assert seen["0"][1] == 2, seen


@pytest.mark.parametrize("s", SCHEDULES, ids=lambda s: "%s%d" % (s[0], s[2]))
def test_many_chunks_and_a_record_larger_than_a_chunk(s):
    data = util.datagen(24 * 131072 + 999, 0.5, 0.0, 8)
    frame = util.compose_frame(data, 10, 1, 1, 1, util.oracle_compress)
    schedule(s)                                             # 2 records per chunk: 13 chunks on 3 stages
    assert fi.index(frame)[4] == 25
    for pinned in (False, True):
        assert decode(frame, len(data), pinned) == (0, len(frame), data), s
    schedule(s, 64 * KIB)                                   # a chunk holds less than one record: every record is a chunk of its own
    short = frame_of_first_records(frame, 7)
    assert decode(short[0], short[1], True) == (0, len(short[0]), data[:short[1]]), s
    ok(s)


def frame_of_first_records(frame, k):
    """(frame with the first k records of `frame`, no checksum and no content size; plain size)."""
    import xxhash
    rc, info, offs, words, n, fb = fi.index(frame)
    hdr = bytes([frame[4] & ~0x0C, frame[5]])
    end = offs[k - 1] + (words[k - 1] & 0x7FFFFFFF)
    return (frame[:4] + hdr + bytes([(xxhash.xxh32(hdr, seed=0).intdigest() >> 8) & 255]) + frame[offs[0] - 4:end] + struct.pack("<I", 0),
            k * util.FRAME_BLOCK_SIZES[info.blockSizeID])


# ---------------------------------------------------------------- errors with chunks in flight ------------------------------------------------

@pytest.mark.parametrize("s", SCHEDULES, ids=lambda s: "%s%d" % (s[0], s[2]))
def test_errors_with_chunks_in_flight(s):
    H = harness()
    data = util.datagen(8 * 131072 + 5, 0.5, 0.0, 44)
    schedule(s)
    good = util.compose_frame(data, 10, 1, 1, 0, util.oracle_compress)          # no content size: the capacity runs out where the bytes do
    linked = fake_frame(data, 10, 1, 1, 0, 0)
    rc, info, offs, words, n, fb = fi.index(good)
    for pinned in (False, True):
        # the capacity runs out in chunk 1 (records 2, 3) while chunks 2 and 3 are issued
        assert decode(good, 3 * 131072 + 100, pinned)[0] == E_TOO_SMALL
        ok(("capacity", s, pinned))
        assert decode(good, len(data), not pinned) == (0, len(good), data)
        # a damaged record in a middle chunk
        for frame, code in ((good, E_GENERIC), (linked, E_FAILED)):
            o = fi.index(frame)[2]
            bad = bytearray(frame)
            bad[o[4] + 1:o[4] + 60] = b"\xff" * 59
            assert decode(bytes(bad), len(data), pinned)[0] == code, (s, pinned, code)
            ok(("damaged", s, pinned))
            assert decode(frame, len(data), pinned) == (0, len(frame), data)
    # the sink of the packed entry runs out of room after some chunks
    bs = 65536
    nb = (len(data) + bs - 1) // bs
    last = len(data) - (nb - 1) * bs
    want = [util.oracle_compress(data[b * bs:(b + 1) * bs], 10) for b in range(nb)]
    cap = sum(len(w) for w in want[:10]) + 5                # chunks of 4 blocks: the third does not fit
    dst = C.create_string_buffer(sum(len(w) for w in want))
    offsets, sizes = (C.c_uint64 * (nb + 1))(), (C.c_uint32 * nb)()
    src = C.create_string_buffer(data, len(data))
    for pinned in (False, True):
        if pinned:
            H.fh_register_pinned(src, len(data))
        assert H.LizardGPU_compressBlocks_host_packed(src, nb, bs, last, dst, cap, offsets, sizes, 10) == -3
        assert b"does not fit" in H.LizardGPU_lastError()
        ok(("sink", s, pinned))
        assert H.LizardGPU_compressBlocks_host_packed(src, nb, bs, last, dst, len(dst), offsets, sizes, 10) == 0
        assert [dst.raw[offsets[b]:offsets[b + 1]] for b in range(nb)] == want and list(sizes) == [len(w) for w in want]
        if pinned:
            H.fh_unregister_pinned(src)
        ok(("after sink", s, pinned))


# ---------------------------------------------------------------- the compress host pipeline ------------------------------------------------

@pytest.mark.parametrize("s", SCHEDULES, ids=lambda s: "%s%d" % (s[0], s[2]))
def test_compress_host_pipeline(s):
    H = harness()
    schedule(s)
    data = util.datagen(21 * 65536 + 12345, 0.5, 0.0, 19) + bytes(70000) + random.Random(9).randbytes(70000)
    for bs, level in ((65536, 10), (131072, 30), (40000, 21)):           # 4 / 2 / 6 blocks per chunk; a ragged last block every time
        nb = (len(data) + bs - 1) // bs
        last = len(data) - (nb - 1) * bs
        want = [util.oracle_compress(data[b * bs:(b + 1) * bs], level) for b in range(nb)]
        stride = util.oracle().lzo_compress_bound(bs)
        src = C.create_string_buffer(len(data) + 8)
        at = C.addressof(src) + 1
        C.memmove(at, data, len(data))
        for pinned in (False, True):
            if pinned:
                H.fh_register_pinned(src, len(src))
            dst = C.create_string_buffer(nb * stride)
            sizes = (C.c_uint32 * nb)()
            assert H.LizardGPU_compressBlocks_host(at, nb, bs, last, dst, stride, sizes, level) == 0, H.LizardGPU_lastError()
            assert [dst.raw[b * stride:b * stride + sizes[b]] for b in range(nb)] == want, (s, bs, pinned)
            packed = C.create_string_buffer(sum(len(w) for w in want))
            offsets = (C.c_uint64 * (nb + 1))()
            assert H.LizardGPU_compressBlocks_host_packed(at, nb, bs, last, packed, len(packed), offsets, None, level) == 0
            assert packed.raw == b"".join(want) and offsets[nb] == len(packed.raw), (s, bs, pinned)
            if pinned:
                H.fh_unregister_pinned(src)
            ok((s, bs, pinned))
        # LizardGPU_decompressBlocks_host hands caller memory to the async copies and synchronises before it returns
        back = C.create_string_buffer(nb * bs)
        out = (C.c_uint32 * nb)()
        H.fh_allow_pageable(1)
        try:
            assert H.LizardGPU_decompressBlocks_host(packed, offsets, nb, back, bs, out) == 0
        finally:
            H.fh_allow_pageable(0)
        assert list(out) == [bs] * (nb - 1) + [last] and b"".join(back.raw[b * bs:b * bs + out[b]] for b in range(nb)) == data, (s, bs)
        ok((s, bs, "decompress"))
    # lzgpu_frame_records through LizardF_compressFrame: byte-equal to the restatement of the frame layer on the oracle
    for level, bsid, checksum, csize in ((10, 1, 1, 0), (30, 2, 0, 1)):
        assert fake_frame(data, level, bsid, checksum, csize, 1) == util.compose_frame(data, level, bsid, checksum, csize, util.oracle_compress), (s, level)
    assert H.pf_degraded() == 0


# ---------------------------------------------------------------- damaged frames ------------------------------------------------

def small_bases():
    """Small frames of many chunks: flushes every few KiB give short records, and a chunk is two records whatever their size."""
    d = util.datagen(60000, 0.5, 0.0, 71)
    t = (b"the quick brown fox jumps over the lazy dog. " * 1000)[:40000]
    mix = d[:15000] + random.Random(5).randbytes(9000) + d[15000:30000]
    cut = lambda n, k: [n // k] * (k - 1) + [n - (n // k) * (k - 1)]
    out = [("flushed L10 crc", fake_flushed(d, cut(len(d), 9), 10, 1, 1, 1)),
           ("flushed L21 linked", fake_flushed(t, cut(len(t), 7), 21, 1, 0, 0)),
           ("flushed L30 mixed", fake_flushed(mix, cut(len(mix), 6), 30, 1, 1, 0)),
           ("flushed L10 linked crc", fake_flushed(d[:30000], cut(30000, 5), 10, 1, 0, 1)),
           ("composed one block size", util.compose_frame(d[:50000], 13, 1, 0, 1, util.oracle_compress))]
    ref = util.reference()
    if ref is not None:
        for mode in (0, 1):
            out.append(("reference fresh mode %d" % mode, util.reference_frame(d + d[:30000], util.frame_prefs(17, 1, 1, 0, mode))))
    return out


def test_differential_on_damaged_frames():
    """tests/test_frame_decompress_gpu.py's damage generator and three-way classification, the fake device in the GPU's place, under
    the random schedule.  The two proportions depend on the host decoder alone (checked first, without the fake)."""
    H = harness()
    seed = tg.SEED
    schedule(("random", RANDOM, seed & 0x7FFFFFFF))
    bases = small_bases() + [("golden linked, 5 records", frame_of_first_records(golden("frame_ref_linked.liz"), 5)[0])]
    per_base = 440 // len(bases) + 1
    rnd = random.Random(seed)
    cases = [(name, ) + tg.damage(rnd, frame) for name, frame in bases for _ in range(per_base)]
    host = [fi.host_one_call(bad, tg.slot_bound(bad)) for _, _, bad in cases]
    accepted = sum(1 for he, hint, _, _ in host if he == 0 and hint == 0)
    refused = sum(1 for he, _, _, _ in host if he)
    assert len(cases) >= 400 and accepted * 100 >= len(cases) and refused * 100 >= 45 * len(cases), (len(cases), accepted, refused)
    counts = collections.Counter()
    saved = tg.lib
    tg.lib = lambda: H                                      # assemble(): the records one by one through the fake's LizardGPU_decompressBlocks_host
    try:
        for total, ((name, kind, bad), (he, hint, hused, hgot)) in enumerate(zip(cases, host)):
            cap = tg.slot_bound(bad)
            ge, gused, ggot = decode(bad, cap, pinned=bool(total & 1))
            what = (name, kind, total, seed)
            ok(what)
            if he == 0 and hint == 0:
                assert ge == 0, (what, "only the host accepts", ge)
                assert (gused, ggot) == (hused, hgot), what
                counts[kind, "both accept"] += 1
            elif ge:
                if he in tg.SAME_CODE:
                    assert ge == he, (what, he, ge)
                counts[kind, "both refuse" if he else "unfinished"] += 1
                if not he:
                    assert ge in (E_GENERIC, 12) or fi.index(bad)[0] == 0, (what, ge)
            else:
                assert he in (E_GENERIC, E_FAILED), (what, he)
                H.fh_allow_pageable(1)
                try:
                    assert tg.assemble(bad) == ggot, what
                finally:
                    H.fh_allow_pageable(0)
                counts[kind, "device only"] += 1
    finally:
        tg.lib = saved
    print("seed %d, %d damaged frames (host decoder: %d accepted, %d refused):" % (seed, len(cases), accepted, refused))
    for k in sorted(counts):
        print("  %-14s %-12s %d" % (k[0], k[1], counts[k]))
    assert sum(counts.values()) == len(cases)


# ---------------------------------------------------------------- sanitizers ------------------------------------------------

def _sanitized(kind):
    try:
        return built(kind)
    except subprocess.CalledProcessError:
        pytest.skip("no %s runtime" % ("ThreadSanitizer" if kind == "tsan" else "AddressSanitizer"))


def test_threads_under_thread_sanitizer():
    """8 threads of mixed frame decodes (pageable and pinned sources) and host-batch compressions on one fake context, random
    schedule: the drain thread of run_host_job, and with chunks above 16 MiB the copy threads of par_memcpy."""
    exe = _sanitized("tsan")
    r = subprocess.run([exe, "threads", "8", "3", "1"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " 0 bad" in r.stdout and "ThreadSanitizer" not in r.stderr, (r.stdout + r.stderr)[-3000:]


def test_core_cases_under_address_sanitizer():
    """Every schedule, both chunk sizes: frames of this library (independent, linked, flushed) from both kinds of source, a damaged
    frame, the compress entries against the oracle.  Device allocations are poisoned while host code runs."""
    exe = _sanitized("asan")
    r = subprocess.run([exe, "core"], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "core: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
