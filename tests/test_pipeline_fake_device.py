"""CPU: LizardGPU_decompressFrame_device / LizardGPU_frameIndex_device (lizard_amd/csrc/lizard_unframe_device.c) as a unit under test
on the fake HIP runtime with DEFERRED streams (tests/fake_hip.c, tests/pipeline_fake.c; see tests/test_pipeline_fake.py).  The walk
is the real lz_unframe_walk body and the records the real lz_unframe_record body on the SIMT emulator; the in-place launch restates
the slot rule of lz_unframe_inplace_kernel, the gather is the plain model of lz_scan_kernel + lz_gather_kernel.  Source and
destination are fake DEVICE allocations with 4 KiB canary margins inside the allocation; the frame and the canary fill are uploaded
with hipMemcpyAsync on a caller's stream that is NOT synchronised before the call, so the entry's ordering behind that stream is
load-bearing under the lazy and random schedules.  The harness is built with LZV_HASH_PIECE = 40961: a 1 MiB frame is hashed in
about 25 pieces through the two alternating pinned buffers.  Every decode is compared with the host twin LizardGPU_decompressFrame on
the same fake and with the plain input (or LizardF_decompress), and ok() — no violation, queues empty at release — follows every call.

Wall time, measured on one machine: the CPU suite at the parent commit 1189 s (225 tests); this module alone 131 s (40 tests; 45 s of
it build the three forms of the harness, which it shares with test_pipeline_fake.py when both run in one session, 26 s are the two
sanitizer programs): below the quarter of the rest of the CPU suite that a fake-device module may take.  The emulated decoder does
about 5 MB/s, which sizes the cases: frames of 0.3 - 1 MiB with 128 KiB blocks, 448 damaged frames of 30 - 90 KB."""
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
import test_frame_decompress_gpu as tg
import test_pipeline_fake as pf
from golden.make_frame_golden import golden_frame_input

G = 4096
CANARY = 0xC3
KIB = 1024
SKIP_CHECKSUM = 1
E_GENERIC, E_TOO_SMALL, E_HEADER_INCOMPLETE, E_FRAMESIZE, E_FAILED, E_CONTENT_CRC = 1, 11, 12, 14, 16, 18
PF_WALK, PF_INPLACE, PF_UNFRAME = 0, 1, 2
H2D, D2H = 1, 2
BLOCK = 131072
SKIP = struct.pack("<II", 0x184D2A57, 9) + b"skippable"
# (LIZARDGPU_WALK_RECORDS, chunk bytes) of each schedule: every budget with both chunk sizes somewhere; tests that depend on one
# combination set it themselves
CONFIG = {("eager", 1): (None, 256 * KIB), ("lazy", 1): ("1", 256 * KIB), ("random", 101): ("2", 1024 * KIB), ("random", 202): ("3", 256 * KIB),
          ("random", 303): ("1", 1024 * KIB)}
SCHEDULES = pf.SCHEDULES
sched_id = lambda s: "%s%d" % (s[0], s[2])


@functools.lru_cache(maxsize=None)
def harness():
    H = pf.harness()
    H.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
    H.hipHostMalloc.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipHostFree.argtypes = [C.c_void_p]
    H.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipStreamCreateWithFlags.argtypes = [C.c_void_p, C.c_uint]
    H.hipStreamSynchronize.argtypes = [C.c_void_p]
    H.LizardGPU_decompressFrame_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_void_p]
    H.LizardGPU_decompressFrame_device.restype = C.c_size_t
    H.LizardGPU_frameIndex_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    H.pf_refuse_launch.argtypes = [C.c_int, C.c_int]
    H.fh_fail_malloc.argtypes = [C.c_int]
    return H


@functools.lru_cache(maxsize=None)
def caller_stream():
    st = C.c_void_p()
    assert harness().hipStreamCreateWithFlags(C.byref(st), 1) == 0
    return st


ok = pf.ok


def configure(s, walk="config", chunk=None):
    cfg = CONFIG[s[0], s[2]]
    walk = cfg[0] if walk == "config" else walk
    pf.schedule(s, chunk or cfg[1])
    if walk is None:
        os.environ.pop("LIZARDGPU_WALK_RECORDS", None)
    else:
        os.environ["LIZARDGPU_WALK_RECORDS"] = walk
    return 4096 if walk is None else int(walk)


@pytest.fixture(autouse=True)
def _no_budget_left_behind():
    yield
    os.environ.pop("LIZARDGPU_WALK_RECORDS", None)
    harness().pf_refuse_launch(PF_WALK, 0); harness().pf_refuse_launch(PF_INPLACE, 0); harness().pf_refuse_launch(PF_UNFRAME, 0)
    harness().fh_fail_malloc(0)


def dstats():
    out = (C.c_ulonglong * 4)()
    assert harness().LizardGPU_frameDecodeDeviceStats(out) == 0
    return list(out)


def grown(s0):
    return [b - a for a, b in zip(s0, dstats())]


class Upload:
    """A fake device allocation: 4 KiB of `fill`, `n` bytes (`data`, or `fill`), 4 KiB of `fill`, written by hipMemcpyAsync from pinned
    memory on the caller's stream and not waited for."""
    def __init__(self, n, fill, data=None):
        H = harness()
        self.n, self.fill, self.size = n, fill, n + 2 * G
        self.dev, self.pin = C.c_void_p(), C.c_void_p()
        assert H.hipMalloc(C.byref(self.dev), self.size) == 0 and H.hipHostMalloc(C.byref(self.pin), self.size, 0) == 0
        C.memset(self.pin, fill, self.size)
        if data:
            C.memmove(self.pin.value + G, bytes(data), n)
        assert H.hipMemcpyAsync(self.dev, self.pin, self.size, H2D, caller_stream()) == 0
        self.at = self.dev.value + G

    def fetch(self, what):
        """The n bytes, once the margins are found intact."""
        H = harness()
        back = C.create_string_buffer(self.size)
        assert H.hipMemcpy(back, self.dev, self.size, D2H) == 0
        raw = back.raw
        assert raw[:G] == bytes([self.fill]) * G and raw[G + self.n:] == bytes([self.fill]) * G, what
        return raw[G:G + self.n]

    def free(self):
        H = harness()
        assert H.hipFree(self.dev) == 0 and H.hipHostFree(self.pin) == 0


def device(frame, cap, flags=0, sync=False, what=None, fail_malloc=0):
    """(error number or 0, consumed, bytes) of the device entry."""
    H = harness()
    src, dst = Upload(len(frame), 0x5A, frame), Upload(cap, CANARY)
    if sync:
        H.hipStreamSynchronize(caller_stream())
    used = C.c_size_t(12345)
    H.fh_fail_malloc(fail_malloc)
    r = H.LizardGPU_decompressFrame_device(dst.at, cap, src.at, len(frame), C.byref(used), flags, caller_stream())
    H.fh_fail_malloc(0)
    ok(("device entry", what, cap, flags))
    body = dst.fetch("the device frame decoder wrote outside d_dst")
    assert src.fetch("the source's margins changed") == bytes(frame), "the source changed"
    src.free(); dst.free()
    e = pf.err_of(r)
    if e:
        assert used.value == 0
        return e, 0, b""
    assert r <= cap
    return 0, used.value, body[:r]


_turn = [0]


def both(frame, cap, what=None):
    """The device entry and the host twin on the same fake: identical, returned once."""
    got = device(frame, cap, what=what)
    _turn[0] += 1
    want = pf.decode(frame, cap, pinned=bool(_turn[0] & 1))
    ok(("host twin", what, cap))
    assert got == want, ("device entry and host twin disagree", what, got[:2], want[:2], cap, len(frame))
    return got


def check_frame(frame, plain, what, B, caps=None, host=True):
    """Capacities exact, the bound, exact + 77, exact - 1; the walk launches of all these calls; LizardF_decompress in one call."""
    b = fi.bound(frame)
    assert not fi.err_of(b) and b >= len(plain), what
    n = fi.index(frame)[4]
    s0 = dstats()
    caps = sorted({len(plain), b, len(plain) + 77}) if caps is None else caps
    for cap in caps:
        e, used, got = both(frame, cap, what)
        assert (e, used) == (0, len(frame)) and got == plain, (what, cap, e, harness().LizardGPU_lastError())
    calls = len(caps)
    if len(plain):
        assert both(frame, len(plain) - 1, what)[0] == E_TOO_SMALL, what
        calls += 1
    d = grown(s0)
    assert d[3] == calls * (n // B + 1), (what, "walk launches", d, calls, n, B)
    if host:
        he, hint, hused, hgot = fi.host_one_call(frame, len(plain) + 16)
        assert (he, hint, hused) == (0, 0, len(frame)) and hgot == plain, what
    return d, calls, n


def with_content_size(frame, size):
    """The frame (15-byte header) with another content size in its header, header checksum redone."""
    import xxhash
    assert frame[4] & 8
    hdr = frame[4:6] + struct.pack("<Q", size)
    return frame[:4] + hdr + bytes([(xxhash.xxh32(hdr, seed=0).intdigest() >> 8) & 255]) + frame[15:]


@functools.lru_cache(maxsize=None)
def data():
    d = util.datagen(4 * BLOCK + 4321, 0.5, 0.0, 97)
    return {"p50": d, "text": (b"the quick brown fox jumps over the lazy dog. " * 9000)[:3 * BLOCK - 17], "noise": random.Random(3).randbytes(300000),
            "mib": util.datagen(8 * BLOCK, 0.5, 0.0, 12)}


# ---------------------------------------------------------------- whole frames ------------------------------------------------

@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_frames_of_this_library(s):
    d = data()
    B = configure(s)
    if s[1] == pf.LAZY:
        harness().pf_shutdown()                             # fresh (poisoned) tables and staging under the schedule that runs everything as late as it may
    seen = []
    for name, plain, level, checksum, csize, mode in (("independent L10 crc size", d["p50"], 10, 1, 1, 1), ("linked L30", d["text"], 30, 0, 0, 0),
                                                      ("linked L10 crc", d["text"], 10, 1, 1, 0), ("independent L30 size", d["p50"][:2 * BLOCK], 30, 0, 1, 1)):
        frame = pf.fake_frame(plain, level, 1, checksum, csize, mode)
        light = name in ("linked L10 crc", "independent L30 size")
        dd, calls, n = check_frame(frame, plain, (name, s), B, caps=[len(plain)] if light else None, host=not light)
        assert dd[2] == 0, "a frame of this library was finished on the host"
        assert dd[0] > 0 and dd[1] == 0, (name, dd)        # only the last record is short: nothing sits in the wrong place
        seen.append((name, n, calls, dd))
    # the header's content size is one the buffer holds, the records are more: the frame is wrong, not the buffer
    frame = pf.fake_frame(d["p50"], 10, 1, 1, 1, 1)
    short = with_content_size(frame, len(d["p50"]) - 1000)
    for cap in (len(d["p50"]) - 1000, len(d["p50"]) - 1, len(d["p50"]), len(d["p50"]) + 50):
        assert both(short, cap, "content size below the records")[0] == E_FRAMESIZE, cap
    assert both(short, len(d["p50"]) - 1001, "content size above the capacity")[0] == E_TOO_SMALL
    assert both(with_content_size(frame, len(d["p50"]) + 1), len(d["p50"]) + 10, "content size above the records")[0] == E_FRAMESIZE
    print("devFrameStats", sched_id(s), "B", B, seen)


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_short_records_in_the_middle_go_through_staging(s):
    d = data()["p50"]
    pieces = [BLOCK, 1, 70000, BLOCK + 1, 5]
    pieces.append(len(d) - sum(pieces))
    for mode in (1, 0):
        # the second round: three records per segment and two per staging chunk, so that one segment needs more than one chunk
        B = configure(s) if mode else configure(s, "3", 256 * KIB)
        frame = pf.fake_flushed(d, pieces, mode=mode)
        assert fi.index(frame)[4] > len(pieces)
        dd, calls, n = check_frame(frame, d, ("flushed", mode, s), B, caps=None if mode else [len(d)], host=bool(mode))
        assert (dd[1] > 0) == (B > 1) and dd[0] > 0 and dd[2] == 0, dd       # a segment of one record starts where it belongs
        print("devFrameStats", sched_id(s), "flushed mode", mode, "B", B, n, calls, dd)


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_capacity_edges_of_the_in_place_pass(s):
    plain = data()["p50"][:3 * BLOCK + 50000]              # (a last record long enough to be stored compressed)
    B = configure(s)
    frame = pf.fake_frame(plain, 10, 1, 1, 0, 1)            # no content size: the capacity runs out where the bytes do
    n = fi.index(frame)[4]
    assert n == 4
    s0 = dstats()
    assert both(frame, len(plain), "the last record fits its short slot exactly") == (0, len(frame), plain)
    d = grown(s0)
    assert d[:3] == [4, 0, 0], d
    s0 = dstats()
    assert both(frame, len(plain) - 1, "one byte short in the last slot")[0] == E_TOO_SMALL
    d = grown(s0)
    assert d[:3] == [3, 0, 0], d                            # the last record fails in place and is refused in staging: nothing gathered
    for cap, what in ((3 * BLOCK + 100, "ends inside the last slot"), (2 * BLOCK, "ends on a slot border with records to come"),
                      (BLOCK, "one slot"), (1, "one byte"), (0, "capacity 0")):
        assert both(frame, cap, what)[0] == E_TOO_SMALL, what
    # the last record damaged: it fails in its (short) slot and again in staging
    offs, words = fi.index(frame)[2:4]
    bad = bytearray(frame)
    bad[offs[3] + 1:offs[3] + 60] = b"\xff" * 59
    for cap in (len(plain), len(plain) + BLOCK):
        assert both(bytes(bad), cap, "the last record damaged")[0] == E_GENERIC, cap
    linked = bytearray(pf.fake_frame(plain, 10, 1, 0, 0, 0))
    o = fi.index(bytes(linked))[2]
    linked[o[3] + 1:o[3] + 60] = b"\xff" * 59
    assert both(bytes(linked), len(plain), "the last record of a linked frame damaged")[0] == E_FAILED
    assert both(frame, len(plain), "a good call after the errors") == (0, len(frame), plain)


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_raw_empty_skippable_and_concatenated_frames(s):
    d = data()
    B = configure(s)
    f_raw = pf.fake_frame(d["noise"], 10, 1, 1, 0, 1)
    assert all(w >> 31 for w in fi.index(f_raw)[3])
    dd, _, _ = check_frame(f_raw, d["noise"], ("all raw", s), B, caps=[len(d["noise"]), len(d["noise"]) + 77])
    assert dd[2] == 0
    flushed = pf.fake_flushed(d["noise"][:250000], [100000, BLOCK, 18928], checksum=0)
    assert all(w >> 31 for w in fi.index(flushed)[3])
    dd, _, _ = check_frame(flushed, d["noise"][:250000], ("raw flushed", s), B, caps=[250000])
    assert (dd[1] > 0) == (B > 1) and dd[2] == 0, dd
    one = pf.fake_frame(b"x", 10, 1, 1, 0, 1)
    check_frame(one, b"x", ("one byte", s), B)
    for checksum in (0, 1):
        empty = pf.fake_frame(b"", 10, 1, checksum, 0, 1)
        s0 = dstats()
        assert both(empty, 0) == (0, len(empty), b"") and both(empty, 100) == (0, len(empty), b"")
        assert grown(s0) == [0, 0, 0, 2]
        for cut in range(1, 5 if checksum else 1):
            assert both(empty[:-cut], 100, "an empty frame cut in its checksum")[0] == E_GENERIC
    s0 = dstats()
    assert both(SKIP, 0) == (0, len(SKIP), b"") and both(SKIP + b"tail", 50) == (0, len(SKIP), b"")
    assert both(SKIP[:-1], 50)[0] == E_GENERIC and both(SKIP[:7], 50)[0] == E_HEADER_INCOMPLETE and both(SKIP[:4], 50)[0] == E_HEADER_INCOMPLETE
    assert grown(s0) == [0, 0, 0, 5]
    small = d["text"][:70000]
    f1 = pf.fake_frame(small, 21, 1, 1, 1, 1)
    stream = SKIP + f1 + f_raw + SKIP + one
    pos, out = 0, []
    while pos < len(stream):
        e, used, got = both(stream[pos:], 1 << 19, "concatenation")
        assert e == 0 and used > 0
        out.append(got)
        pos += used
    assert out == [b"", small, d["noise"], b"", b"x"] and pos == len(stream)


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_content_checksum_in_many_pieces_and_the_skip_flag(s):
    """1 MiB in 8 records: 26 pieces of 40961 bytes a call; with a budget of 1 - 3 records the pieces of a segment are copied and hashed
    while the next segment decodes."""
    plain = data()["mib"]
    B = configure(s)
    for mode in ((1, 0) if s[2] in (1, 202) else (1,)):
        frame = pf.fake_frame(plain, 10, 1, 1, 0, mode)
        assert frame[4] & 4 and fi.index(frame)[4] == 8
        assert both(frame, len(plain), "checksum") == (0, len(frame), plain)
        assert device(frame, len(plain), SKIP_CHECKSUM) == (0, len(frame), plain)
        bad = frame[:-2] + bytes([frame[-2] ^ 0x10]) + frame[-1:]
        assert both(bad, len(plain), "stored checksum flipped")[0] == E_CONTENT_CRC
        assert device(bad, len(plain), SKIP_CHECKSUM) == (0, len(frame), plain)
        inner = bytearray(frame)
        inner[fi.index(frame)[2][5] + 40] ^= 0x01              # most damage to a payload changes bytes, not the structure
        e = both(bytes(inner), len(plain), "payload bit flipped")
        assert e[0] in (E_CONTENT_CRC, E_GENERIC, E_FAILED)
        for cut in (1, 3, 4):
            for flags in (0, SKIP_CHECKSUM):
                assert device(frame[:-cut], len(plain), flags)[0] == E_GENERIC, (cut, flags)
        assert both(frame[:-2], len(plain), "cut inside the checksum")[0] == E_GENERIC
    # a short frame: fewer bytes than one piece, and one byte more than two pieces
    for n in (40960, 2 * 40961 + 1):
        frame = pf.fake_frame(plain[:n], 10, 1, 1, 1, 1)
        assert both(frame, n, "short checksummed frame") == (0, len(frame), plain[:n])


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_reference_made_golden_frames(s):
    plain = golden_frame_input()
    B = configure(s)
    linked, independent = pf.golden("frame_ref_linked.liz"), pf.golden("frame_ref_independent.liz")
    assert linked[4] & 4
    s0 = dstats()
    assert both(linked, len(plain), "golden linked") == (0, len(linked), plain)
    assert device(linked, len(plain), SKIP_CHECKSUM) == (0, len(linked), plain)
    bad = linked[:-1] + bytes([linked[-1] ^ 1])
    assert both(bad, len(plain), "golden linked, checksum flipped")[0] == E_CONTENT_CRC
    assert device(bad, len(plain), SKIP_CHECKSUM) == (0, len(linked), plain)
    assert both(linked, len(plain) - 1, "golden linked, one byte short")[0] == E_TOO_SMALL
    d = grown(s0)
    assert d[2] == 5, ("every decode of the reference's linked frame is finished on the host", d)
    n = fi.index(independent)[4]
    dd, calls, _ = check_frame(independent, plain, ("golden independent", s), B, caps=[len(plain)], host=False)
    assert dd[2] == 0 and dd[0] >= n, dd
    print("devFrameStats", sched_id(s), "golden linked", d, "independent", dd)


# ---------------------------------------------------------------- failures of the machinery ------------------------------------------------

@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_a_call_that_fails_in_the_machinery_then_a_good_call(s):
    H = harness()
    d = data()["p50"]
    configure(s, "2")
    good = pf.fake_frame(d, 10, 1, 1, 0, 1)
    pieces = [BLOCK, 1, 70000, BLOCK + 1, len(d) - 2 * BLOCK - 70002]      # two records per segment: the 4th and the 6th record go through staging
    flushed = pf.fake_flushed(d, pieces)
    for kind, nth, frame in ((PF_WALK, 1, good), (PF_WALK, 2, good), (PF_WALK, 3, flushed), (PF_INPLACE, 1, good), (PF_INPLACE, 2, good),
                             (PF_UNFRAME, 1, flushed), (PF_UNFRAME, 2, flushed)):
        H.pf_refuse_launch(kind, nth)
        got = device(frame, len(d), what=("refused launch", kind, nth))      # ok() inside: nothing left in flight
        assert got == (E_GENERIC, 0, b""), (kind, nth, got)
        assert b"refused by the test" in H.LizardGPU_lastError()
        assert both(frame, len(d), "after a refused launch") == (0, len(frame), d)
    # the tables, then the staging slots cannot be allocated (the caller's stream is synchronised here: a call that fails before it
    # orders itself behind that stream leaves the caller's own work queued, as it may)
    for nth, frame in ((1, good), (1, flushed), (2, flushed)):
        H.pf_shutdown()
        H.hipStreamSynchronize(caller_stream())
        got = device(frame, len(d), sync=True, what=("hipMalloc fails", nth), fail_malloc=nth)
        assert got == (E_GENERIC, 0, b""), (nth, got)
        assert both(frame, len(d), "after a failed allocation") == (0, len(frame), d)


# ---------------------------------------------------------------- damaged frames ------------------------------------------------

@functools.lru_cache(maxsize=None)
def damaged_cases():
    """test_pipeline_fake.py's damaged frames, with its seed: bases built inside the fake, tests/test_frame_decompress_gpu.py's generator."""
    seed = tg.SEED
    pf.schedule(("random", pf.RANDOM, seed & 0x7FFFFFFF))
    bases = pf.small_bases() + [("golden linked, 5 records", pf.frame_of_first_records(pf.golden("frame_ref_linked.liz"), 5)[0])]
    per_base = 440 // len(bases) + 1
    rnd = random.Random(seed)
    return seed, bases, [(name, ) + tg.damage(rnd, frame) for name, frame in bases for _ in range(per_base)]


def test_differential_on_damaged_frames():
    seed, bases, cases = damaged_cases()
    host = [fi.host_one_call(bad, tg.slot_bound(bad)) for _, _, bad in cases]
    accepted = sum(1 for he, hint, _, _ in host if he == 0 and hint == 0)
    refused = sum(1 for he, _, _, _ in host if he)
    assert len(cases) >= 400 and accepted * 20 >= len(cases) and refused * 20 >= len(cases), (len(cases), accepted, refused)
    counts, errors = collections.Counter(), collections.Counter()
    pf.schedule(("random", pf.RANDOM, seed & 0x7FFFFFFF))
    s0 = dstats()
    for i, ((name, kind, bad), (he, hint, hused, hgot)) in enumerate(zip(cases, host)):
        budget = (None, "1", "2", "3")[i & 3]
        if budget is None:
            os.environ.pop("LIZARDGPU_WALK_RECORDS", None)
        else:
            os.environ["LIZARDGPU_WALK_RECORDS"] = budget
        e, used, got = both(bad, tg.slot_bound(bad), (name, kind, i, seed))
        if he == 0 and hint == 0:
            assert (e, used, got) == (0, hused, hgot), (name, kind, i, seed)
        counts[kind, "accepted" if e == 0 else "refused"] += 1
        errors[e] += 1
    print("seed %d, %d damaged frames (host decoder: %d accepted, %d refused); device entry = host twin on all; devFrameStats %s"
          % (seed, len(cases), accepted, refused, grown(s0)))
    for k in sorted(counts):
        print("  %-14s %-9s %d" % (k[0], k[1], counts[k]))
    print("  by error number:", dict(sorted(errors.items())))
    assert sum(counts.values()) == len(cases) and errors[0] >= accepted


# ---------------------------------------------------------------- LizardGPU_frameIndex_device ------------------------------------------------

def device_index(frame, max_records=None, tables=True):
    """fi.index through LizardGPU_frameIndex_device: (rc, info, offsets, words, nRecords, frameBytes); guard words around the tables."""
    H = harness()
    info = util.FrameInfo()
    n, fb = C.c_size_t(0), C.c_size_t(0)
    src = Upload(len(frame), 0x5A, frame)
    rc = H.LizardGPU_frameIndex_device(src.at, len(frame), C.byref(info), None, None, 0, C.byref(n), C.byref(fb), caller_stream())
    ok("frameIndex_device without tables")
    if rc or not tables:
        src.free()
        return rc, info, [], [], n.value, fb.value
    m = n.value if max_records is None else max_records
    t = Upload(12 * m + 24, 0xF9)                               # [8 guard][m offsets][8 guard] and [4 guard][m words][4 guard] behind it
    o_at, w_at = t.at + 8, t.at + 8 + 8 * m + 8 + 4
    rc = H.LizardGPU_frameIndex_device(src.at, len(frame), C.byref(info), o_at, w_at, m, C.byref(n), C.byref(fb), caller_stream())
    ok("frameIndex_device with tables")
    raw = t.fetch("the index wrote outside its tables")
    k = min(m, n.value)
    offs = list(struct.unpack_from("<%dQ" % m, raw, 8)) if m else []
    words = list(struct.unpack_from("<%dI" % m, raw, 8 + 8 * m + 8 + 4)) if m else []
    guards = raw[:8] + raw[8 + 8 * m:8 + 8 * m + 12] + raw[-4:] + struct.pack("<%dQ" % (m - k), *offs[k:]) + struct.pack("<%dI" % (m - k), *words[k:])
    assert guards == b"\xf9" * len(guards), "the index wrote outside the records it found"
    src.free(); t.free()
    return rc, info, offs[:k], words[:k], n.value, fb.value


def same_index(a, b):
    fields = lambda i: (i.blockSizeID, i.blockMode, i.contentChecksumFlag, i.frameType, i.contentSize)
    return (a[0], fields(a[1])) + tuple(a[2:]) == (b[0], fields(b[1])) + tuple(b[2:])


@pytest.mark.parametrize("s", [SCHEDULES[1], SCHEDULES[3]], ids=sched_id)
def test_frame_index_device_matches_the_host_walk(s):
    seed, bases, cases = damaged_cases()
    pf.schedule(s)
    intact = [f for _, f in bases] + [SKIP, SKIP + b"x", pf.fake_frame(b"", 10, 1, 1, 0, 1)]
    for f in intact:
        assert same_index(device_index(f), fi.index(f))
        assert same_index(device_index(f + b"\x04\x22\x4d\x18tail"), fi.index(f + b"\x04\x22\x4d\x18tail"))
        for m in (0, 1, 3):
            assert same_index(device_index(f, m), fi.index(f, m)), m
        got, want = device_index(f, tables=False), fi.index(f)
        assert (got[0], got[4], got[5]) == (want[0], want[4], want[5])
    counts = collections.Counter()
    for i, (name, kind, bad) in enumerate(cases):
        if (i + s[2]) % 2:
            continue
        want = fi.index(bad, (None, 0, 1, 3)[(i // 2) & 3])
        assert same_index(device_index(bad, (None, 0, 1, 3)[(i // 2) & 3]), want), (name, kind, i)
        counts[want[0]] += 1
    print("frameIndex_device on damaged frames:", dict(counts))
    assert counts[0] > 10 and sum(counts.values()) - counts[0] > 10, counts


# ---------------------------------------------------------------- sanitizers ------------------------------------------------

def test_device_entry_core_cases_under_address_sanitizer():
    """Every schedule, budgets 1 / 2 / 3 / unset and both chunk sizes: independent, linked and flushed frames with checksum in pieces,
    the capacity edges, a damaged frame, a refused launch.  Device allocations are poisoned while host code runs, so host code of the
    entry that dereferenced d_src / d_dst or its device tables would fault."""
    exe = pf._sanitized("asan")
    r = subprocess.run([exe, "devcore"], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "devcore: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_device_entry_threads_under_thread_sanitizer():
    """6 threads mixing the device entry, the host twin and a host-batch compression on one fake context under the random schedule."""
    exe = pf._sanitized("tsan")
    r = subprocess.run([exe, "devthreads", "6", "3"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " 0 bad" in r.stdout and "ThreadSanitizer" not in r.stderr, (r.stdout + r.stderr)[-3000:]
