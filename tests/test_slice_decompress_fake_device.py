"""CPU: LizardGPU_decompressFrameRanges_device (lizard_amd/csrc/lizard_slice_device.c, compiled as it is) as a unit under test on the fake
HIP runtime with DEFERRED streams: tests/slice_device_fake.c (the unit and plain sequential models of its own two launches; records
decode through the emulator's objects) linked with tests/unframes_device_fake.c (the model of the walk launch the unit reuses: the real
walk on the emulator), tests/pipeline_fake.c and tests/fake_hip.c as they are.  Everything behind the count pass is enqueued before the
host waits again, so under the lazy and random schedules a missing order — the decode before the record tables are filled, the
per-pick results read back too early — is wrong answers on every run.
Frames of 0 - 3 blocks of 128 KiB; ranges inside one block, across a block edge, ending at the content size, empty, two sharing a
block.  sdf_run compares every range of every answered frame with the FULL decode of LizardGPU_decompressFrame_device on the same fake
(bytes at rangeAt[r] + lo % B), and the tests check rangeAt, results and LizardGPU_sliceDeviceStats.  One refusal per rule; a corrupt
block that is NOT picked leaves the answer intact; a capacity one byte short launches nothing and leaves d_dst intact.  ok() — no
violation of the fake's rules, queues empty — follows every call."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_pipeline_fake as pf
import test_frames_decompress_fake_device as fd
import planes_inputs as pi
import bitplanes_inputs as bi

HERE = pf.HERE
B = 131072
ERR_ARG = 3
E_GENERIC, E_FAILED, E_TYPE, E_SIZE = 1, 16, 13, 14
SCHEDULES = [s for s in pf.SCHEDULES if s[1] in (pf.LAZY, pf.RANDOM)]


@functools.lru_cache(maxsize=None)
def built(kind):
    """'lib': the harness as a shared library; 'asan': its program under AddressSanitizer + UBSan.  The emulator's objects are the ones in
    pf._dir, whichever module built them first."""
    return util.build_fake(pf._dir, kind, "slice_device_fake", ("slice_device_fake.c", "unframes_device_fake.c", "pipeline_fake.c", "fake_hip.c"),
                           csrc=("lizard_slice_host.c",) + util.FAKE_CSRC)


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built("lib"))
    H.fh_set_abort(0)
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.sdf_last_error.restype = C.c_char_p
    H.sdf_launches.argtypes = [C.c_int]; H.sdf_launches.restype = C.c_ulonglong
    H.sdf_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]; H.sdf_frame.restype = C.c_size_t
    H.sdf_flushed_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]; H.sdf_flushed_frame.restype = C.c_size_t
    H.sdf_run.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    H.sdf_join.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p]
    H.LizardF_isError.argtypes = [C.c_size_t]; H.LizardF_isError.restype = C.c_uint
    H.fh_set_schedule(pf.LAZY, 1)
    return H


def ok(what=""):
    buf = C.create_string_buffer(512)
    n = harness().fh_violations(buf, 512)
    assert n == 0, (what, n, buf.value)


@functools.lru_cache(maxsize=None)
def frame(off, n, level=10, checksum=0, csize=1):
    H = harness()
    buf = C.create_string_buffer(n + n // 8 + 4096)
    got = H.sdf_frame(buf, len(buf), off, n, level, checksum, csize)
    ok("sdf_frame")
    assert not H.LizardF_isError(got), got
    return buf.raw[:got]


def run(frames, ranges_per_frame, cap=None, what=None, refs=None):
    """One call (sdf_run: the bytes of every answered frame's ranges against the full decode).  ranges_per_frame: a list of (lo, hi) per
    frame.  cap None: exactly the room of all ranges.  refs: per frame None or the frame whose full decode is the reference instead.  (rc, error numbers per frame, rangeAt, growth of the statistics, unslice launches)"""
    H = harness()
    nf = len(frames)
    flat = [r for rs in ranges_per_frame for r in rs]
    first = np.cumsum([0] + [len(rs) for rs in ranges_per_frame])[:-1]
    if cap is None:
        cap = room(flat)
    keep = [C.create_string_buffer(bytes(f), max(len(f), 1)) for f in frames]
    ptrs = (C.c_void_p * nf)(*[C.addressof(k) for k in keep])
    sizes = (C.c_size_t * nf)(*[len(f) for f in frames])
    arr = (C.c_uint64 * max(2 * len(flat), 1))(*[v for r in flat for v in r])
    results, range_at, grown, rc = (C.c_size_t * nf)(), (C.c_uint64 * (len(flat) + 1))(), (C.c_ulonglong * 4)(), C.c_int(77)
    refs = [None] * nf if refs is None else refs
    rkeep = [None if f is None else C.create_string_buffer(bytes(f), len(f)) for f in refs]
    rptrs = (C.c_void_p * nf)(*[None if k is None else C.addressof(k) for k in rkeep])
    rsizes = (C.c_size_t * nf)(*[0 if f is None else len(f) for f in refs])
    before = H.sdf_launches(0)
    bad = H.sdf_run(nf, ptrs, sizes, (C.c_uint32 * nf)(*[int(v) for v in first]), (C.c_uint32 * nf)(*[len(rs) for rs in ranges_per_frame]), len(flat), arr,
                    cap, results, range_at, grown, C.byref(rc), rptrs, rsizes)
    ok(what)
    assert bad == 0, (what, H.sdf_last_error())
    return rc.value, [(1 << 64) - r if H.LizardF_isError(r) else int(r) for r in results], list(range_at), list(grown), H.sdf_launches(0) - before


def blocks(r):
    return (-(-r[1] // B) - r[0] // B) if r[1] > r[0] else 0


def room(ranges):
    return sum(blocks(r) * B for r in ranges)


# frames: 3 blocks (the middle one stored raw), 2 blocks + 1 byte, one short block, no blocks
GOOD = [(0, 3 * B), (3 * B, 2 * B + 1), (6 * B, B - 100), (0, 0)]
RANGES = [[(100, 2000), (B - 10, B + 10), (2 * B + 5, 3 * B), (7, 7), (B + 100, B + 200), (B + 150, B + 300)],   # inside, across an edge, ending at C, empty, two sharing a block
          [(2 * B, 2 * B + 1), (0, 2 * B + 1)],                                                                    # the one-byte last block; everything
          [(0, B - 100), (50, 60)],
          [(0, 0)]]


@pytest.mark.parametrize("s", SCHEDULES, ids=fd.sched_id)
def test_ranges_hold_the_bytes_of_the_full_decode(s):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    level = 30 if s[2] in (202, 303) else 10
    frames = [frame(off, n, level, i & 1, 1 if n else 0) for i, (off, n) in enumerate(GOOD)]
    rc, res, at, grown, launches = run(frames, RANGES, what=fd.sched_id(s))
    flat = [r for rs in RANGES for r in rs]
    assert rc == 0 and res == [0, 0, 0, 0] and H.sdf_last_error() == b"", (rc, res, H.sdf_last_error())
    assert at == list(np.cumsum([0] + [blocks(r) * B for r in flat])), at
    picks = sum(blocks(r) for r in flat)
    assert picks == 1 + 2 + 1 + 0 + 1 + 1 + 1 + 3 + 1 + 1 and grown == [picks, 4, 0, 1] and launches == 1, (grown, launches)
    # room to spare changes nothing; only empty ranges: nothing is launched
    rc, res, at2, grown, launches = run(frames, RANGES, cap=room(flat) + 12345)
    assert rc == 0 and res == [0] * 4 and at2 == at
    rc, res, at, grown, launches = run(frames[:2], [[(5, 5)], []], cap=0)
    assert rc == 0 and res == [0, 0] and at == [0, 0] and grown == [0, 2, 0, 1] and launches == 0
    H.fh_set_schedule(pf.LAZY, 1)


def corrupt(f, block=0):
    """40 bytes of 0xFF over the start of the payload of record `block` (frames with content size: a 15-byte header)."""
    at = 15
    for _ in range(block):
        at += 4 + (int.from_bytes(f[at:at + 4], "little") & 0x7FFFFFFF)
    return f[:at + 4 + 3] + b"\xFF" * 40 + f[at + 4 + 3 + 40:]


@pytest.mark.parametrize("s", SCHEDULES[:2], ids=fd.sched_id)
def test_one_refusal_per_rule_and_the_others_are_answered(s):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    good = frame(0, 3 * B)
    flushed = C.create_string_buffer(3 * B)
    n = H.sdf_flushed_frame(flushed, len(flushed), 6 * B, 70000, 70000 + B, 10)
    ok("sdf_flushed_frame")
    assert not H.LizardF_isError(n)
    skippable = bytes([0x57, 0x2A, 0x4D, 0x18, 5, 0, 0, 0]) + b"skip!"
    frames = [good, frame(0, B, csize=0), skippable, frame(0, 2 * B)[:len(frame(0, 2 * B)) // 2], good, corrupt(good, 0), flushed.raw[:n], good, good]
    ranges = [[(10, 20)], [(0, 10)], [(0, 1)], [(0, 10)], [(0, 3 * B + 1)], [(5, 6), (2 * B, 2 * B + 9)], [(0, 100)], [(9, 8)], [(3 * B - 1, 3 * B)]]
    rc, res, at, grown, launches = run(frames, ranges, cap=5 * B, what="refusals")
    assert rc == 0 and launches == 1, (rc, H.sdf_last_error())
    assert res[0] == 0 and res[8] == 0
    assert res[1] == E_SIZE, "no content size"
    assert res[2] == E_TYPE, "a skippable frame"
    assert res[3] == E_GENERIC, "a chain cut in the middle: the walk's own code"
    assert res[4] == E_SIZE and res[7] == E_SIZE, "hi > C, lo > hi"
    assert res[5] == E_FAILED, "a corrupt picked block"
    assert res[6] == E_FAILED, "a flushed frame whose short record is picked"
    assert b"frame 1 refused: ERROR_frameSize_wrong" in H.sdf_last_error()
    # the refused-at-the-count-pass frames take no room; the two that fail in the decode keep theirs
    assert at == [0, B, B, B, B, B, 2 * B, 3 * B, 4 * B, 4 * B, 5 * B], at
    assert grown == [5, 2, 7, 1], grown
    H.fh_set_schedule(pf.LAZY, 1)


def test_damage_outside_the_picked_blocks_is_not_seen():
    """The stated limit: a corrupt block that is NOT picked leaves the answer intact — and the same frame with that block picked is refused."""
    good = frame(0, 3 * B)
    bad = corrupt(good, 0)
    # (the single entry refuses the damaged frame: the reference of sdf_run is the intact frame's full decode)
    rc, res, at, grown, launches = run([bad], [[(B + 5, 3 * B)]], refs=[good])
    assert rc == 0 and res == [0] and grown == [2, 1, 0, 1], (rc, res, grown)
    rc, res, _, _, _ = run([bad], [[(5, 3 * B)]])
    assert rc == 0 and res == [E_FAILED]


def test_a_capacity_one_byte_short_launches_nothing_and_leaves_the_canaries_intact():
    H = harness()
    frames = [frame(off, n, 10, 0, 1 if n else 0) for off, n in GOOD]
    flat = [r for rs in RANGES for r in rs]
    for cap in (room(flat) - 1, 0):
        rc, res, at, grown, launches = run(frames, RANGES, cap=cap, what=("short", cap))      # (sdf_run: a failed call leaves every byte of d_dst as it was)
        assert rc == -ERR_ARG and launches == 0 and b"dstMaxSize_tooSmall" in H.sdf_last_error(), (rc, launches, H.sdf_last_error())
        assert res == [E_GENERIC] * 4 and grown[:3] == [0, 0, 0], (res, grown)
    # a frame refused in the count pass keeps its code
    rc, res, _, _, launches = run(frames[:1] + [frame(0, B, csize=0)], [RANGES[0], [(0, 1)]], cap=room(RANGES[0]) - 1)
    assert rc == -ERR_ARG and res == [E_GENERIC, E_SIZE] and launches == 0
    # bad arguments: a range of two frames
    first = (C.c_uint32 * 2)(0, 0)
    results, range_at, grown, rcv = (C.c_size_t * 2)(), (C.c_uint64 * 2)(), (C.c_ulonglong * 4)(), C.c_int(77)
    keep = [C.create_string_buffer(f, len(f)) for f in frames[:2]]
    got = H.sdf_run(2, (C.c_void_p * 2)(*[C.addressof(k) for k in keep]), (C.c_size_t * 2)(*[len(f) for f in frames[:2]]), first, (C.c_uint32 * 2)(1, 1), 1,
                    (C.c_uint64 * 2)(0, 10), B, results, range_at, grown, C.byref(rcv), None, None)
    ok("a shared range")
    assert got == 0 and rcv.value == -ERR_ARG and b"belongs to frame" in H.sdf_last_error()


@pytest.mark.parametrize("filt", (0, 1), ids=("bytes", "bits"))
def test_the_range_join_on_the_fake(filt):
    """LizardGPU_joinPlanesRange_device's host side (argument checks, table, piece addresses) with the harness's element-by-element model
    of the kernel: join(split)[first * E : last * E], with and without a base.  (The kernel itself: tests/test_planes_range_emul.py.)"""
    H = harness()
    rng = np.random.RandomState(5)
    for E in (1, 2, 4, 8):
        n = 300 + E
        src = rng.randint(0, 256, n * E, dtype=np.uint8)
        split = (bi.bits_split_model if filt else pi.split_model)(src, E)
        for first, last in ((0, n), (3, 200), (n - n % 8 - 2, n), (17, 18), (n - 1, n)):
            for base in (None, rng.randint(0, 256, (last - first) * E, dtype=np.uint8)):
                out = C.create_string_buffer((last - first) * E)
                rc = H.sdf_join(split.tobytes(), split.size, n, E, filt, first, last, None if base is None else base.tobytes(), out)
                ok(("join", E, filt, first, last))
                want = src[first * E:last * E] if base is None else src[first * E:last * E] ^ base
                assert rc == 0 and out.raw == want.tobytes(), (rc, E, filt, first, last, base is not None, H.sdf_last_error())
    out = C.create_string_buffer(64)
    assert H.sdf_join(bytes(64), 64, 8, 8, 2, 0, 8, None, out) == 1000 and H.sdf_join(bytes(64), 64, 8, 8, 0, 0, 0, None, out) == 0
    ok("join refusals")


def test_the_harness_program_under_address_sanitizer():
    """tests/slice_device_fake.c's own main as a program of its own: four schedules, levels 10 and 30, good and refused frames in one
    batch, a capacity one byte short, with device allocations poisoned while host code runs."""
    try:
        exe = built("asan")
    except subprocess.CalledProcessError:
        pytest.skip("no AddressSanitizer runtime")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "slice_device_fake: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
