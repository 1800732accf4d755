"""The batch bodies of LizardGPU_decompressFrames_device (lizard_amd/csrc/unframes_kernels.h: the walk wrapper, settle, finish) on the
CPU SIMT emulator, under both lane schedules.  A batch of frames with 0, 1, 63, 64, 65 and 130 records (raw 1-byte records, assembled
here), entries that are not to be walked and a damaged frame between them: the walk's results are the host walk's, the tables land at
each frame's base and nowhere else, settle agrees with a sequential model, finish with the host's Lizard_XXH32 and the content-size
rule, and no read falls outside a frame's bytes."""
import ctypes as C
import functools
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_unframe_walk_emul as we

EMUL = we.EMUL
SEEDS = we.SEEDS
COUNTS = (0, 1, 63, 64, 65, 130)
WALK, DECODE, VERIFY = 1, 2, 4
DEAD, CLEAN, DELEGATE = 0, 1, 2
ERR, NEED_HISTORY = 0xFFFFFFFF, 0xFFFFFFFE
GAP = 3                                                          # table entries between two frames' regions, and at both ends
SENTINEL64, SENTINEL32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5


class Entry(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("src", "srcSize", "dst", "cap", "first", "contentSize", "frameBytes")] \
             + [(n, C.c_uint32) for n in ("nRecords", "maxBlock", "flags", "reserved")]


class Result(C.Structure):
    _fields_ = [("size", C.c_uint64), ("state", C.c_uint32), ("reserved", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libunframes_emul.so from simt.cpp + unframes_api.cpp, the way test_unframe_walk_emul.py builds its library."""
    out = os.path.join(EMUL, "libunframes_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "unframes_api.cpp")]
    deps = srcs + [os.path.join(EMUL, "lz_wave.h")] + [os.path.join(util.ROOT, "lizard_amd", "csrc", h) for h in ("unframe_walk.h", "unframes_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_unframes_walk.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.emul_unframes_walk.restype = None
    L.emul_unframes_settle.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.emul_unframes_settle.restype = None
    L.emul_unframes_finish.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]
    L.emul_unframes_finish.restype = None
    return L


def test_the_entry_is_the_one_the_host_file_fills():
    assert C.sizeof(Entry) == 72 and C.sizeof(Result) == 16 and C.sizeof(we.WalkResult) == 64


def batch_frames():
    """(frame, walked): the six record counts with both header sizes and checksum on and off, an entry that is not walked in the
    middle, a frame whose chain is cut, a skippable frame."""
    out = [(we.raw_frame([1] * n, 1, i & 1, (i >> 1) & 1, seed=7 + i), True) for i, n in enumerate(COUNTS)]
    cut = we.raw_frame([1] * 65, 1, 1, 0)
    return out[:3] + [(we.raw_frame([1] * 9), False)] + out[3:] + [(cut[:len(cut) - 9], True), (we.SKIP, True)]


def place(frames):
    """The frames in one buffer, 64 bytes of 0x5A around each, frame i starting i bytes off an 8-byte boundary: (buffer, addresses)."""
    pos, at = 64, []
    for i, f in enumerate(frames):
        pos += (8 - pos % 8) % 8 + i % 8
        at.append(pos)
        pos += len(f) + 64
    buf = (C.c_ubyte * pos)()
    C.memset(buf, 0x5A, pos)
    for f, a in zip(frames, at):
        C.memmove(C.addressof(buf) + a, bytes(f), len(f))
    return buf, [C.addressof(buf) + a for a in at]


def test_the_batch_walk_counts_and_fills_each_frame_at_its_base():
    L = lib()
    cases = batch_frames()
    frames = [f for f, _ in cases]
    F = len(frames)
    buf, addr = place(frames)
    hosts = [we.host(f) for f in frames]
    for seed in SEEDS:
        # count mode: every walked entry gets the host walk's answer, the others are left alone
        entries = (Entry * F)()
        for e, f, a, (_, walked) in zip(entries, frames, addr, cases):
            e.src, e.srcSize, e.flags = a, len(f), WALK if walked else 0
        res, spans = (we.WalkResult * F)(), (C.c_longlong * (2 * F))()
        C.memset(res, 0xEE, C.sizeof(res))
        L.emul_unframes_walk(entries, F, 0, None, None, res, spans, seed)
        for i, (r, f, h, (_, walked)) in enumerate(zip(res, frames, hosts, cases)):
            assert 0 <= spans[2 * i] <= spans[2 * i + 1] <= len(f), ("the walk read outside frame", i, list(spans[2 * i:2 * i + 2]), len(f))
            if not walked:
                assert bytes(r) == b"\xEE" * 64 and spans[2 * i + 1] == 0, "an entry that is not to be walked was"
                continue
            assert -r.status == h[0], (i, r.status, h[0])
            if not r.status:
                assert (r.nRecords, r.frameBytes, r.done) == (h[4], h[5], 1), i
                if r.frameType == 0:
                    assert (r.blockSizeID, r.blockMode, r.checksumFlag, r.contentSize) == (h[1][0], h[1][1], h[1][2], h[1][4]), i
        assert [r.nRecords for r, (_, w) in zip(res, cases) if w and not r.status] == list(COUNTS) + [0]
        # fill mode: the accepted normal frames, each at its base, a gap between the regions; one frame with room for one record less
        first, live = GAP, []
        for i, (e, r, (_, walked)) in enumerate(zip(entries, res, cases)):
            e.flags = 0
            if walked and not r.status and not r.frameType:
                e.flags, e.first, e.nRecords = DECODE, first, r.nRecords - (1 if r.nRecords == 64 else 0)
                live.append(i)
                first += r.nRecords + GAP
        total = first
        offs, words = (C.c_uint64 * total)(*([SENTINEL64] * total)), (C.c_uint32 * total)(*([SENTINEL32] * total))
        res2 = (we.WalkResult * F)()
        C.memset(res2, 0xEE, C.sizeof(res2))
        L.emul_unframes_walk(entries, F, 1, offs, words, res2, spans, seed)
        want_o, want_w = [SENTINEL64] * total, [SENTINEL32] * total
        for i in live:
            e, h = entries[i], hosts[i]
            want_o[e.first:e.first + e.nRecords] = h[2][:e.nRecords]
            want_w[e.first:e.first + e.nRecords] = h[3][:e.nRecords]
            assert 0 <= spans[2 * i] <= spans[2 * i + 1] <= len(frames[i])
            assert (res2[i].status, res2[i].nRecords, res2[i].frameBytes) == (0, h[4], h[5])
        assert list(offs) == want_o and list(words) == want_w, "a table entry outside a frame's region changed, or one inside is wrong"
        assert all(bytes(res2[i]) == b"\xEE" * 64 for i in range(F) if i not in live)
        assert len(live) == len(COUNTS)


def settle_model(n, out, max_block):
    bad = any(v >= NEED_HISTORY or (i + 1 < n and v != max_block) for i, v in enumerate(out))
    return (DELEGATE, 0) if bad else (CLEAN, sum(out))


def settle_cases():
    """(what, nRecords, per-record results)."""
    B = 131072
    for n in COUNTS:
        yield "all full", n, [B] * n
        if n:
            yield "short last", n, [B] * (n - 1) + [B - 5]
            yield "empty last", n, [B] * (n - 1) + [0]
            for at in sorted({0, n // 2, n - 1}):
                for what, v in (("a failure", ERR), ("a need-history mark", NEED_HISTORY)):
                    yield "%s at %d" % (what, at), n, [B] * at + [v] + [B] * (n - at - 1)
        if n > 1:
            for at in sorted({0, n // 2, n - 2}):
                yield "short middle at %d" % at, n, [B] * at + [B - 1] + [B] * (n - at - 1)
            yield "oversize middle", n, [B + 1] + [B] * (n - 1)


def test_settle_against_a_sequential_model():
    L = lib()
    B = 131072
    cases = list(settle_cases())
    cases.insert(4, ("not to be decoded", 5, [B] * 5))
    F = len(cases)
    entries, out, first = (Entry * F)(), [], GAP
    for e, (what, n, rec) in zip(entries, cases):
        e.first, e.nRecords, e.maxBlock, e.flags = first, n, B, WALK if what == "not to be decoded" else DECODE | VERIFY
        out += [ERR] * (first - len(out)) + rec                    # (the gaps hold failures: a frame that looks beside its region is not clean)
        first += n + GAP
    out += [ERR] * GAP
    d_out = (C.c_uint32 * len(out))(*out)
    seen = set()
    for seed in SEEDS:
        results, hash_bytes = (Result * F)(), (C.c_uint64 * F)(*([SENTINEL64] * F))
        C.memset(results, 0xEE, C.sizeof(results))
        L.emul_unframes_settle(entries, F, d_out, results, hash_bytes, seed)
        for r, hb, (what, n, rec) in zip(results, hash_bytes, cases):
            want = (DEAD, 0) if what == "not to be decoded" else settle_model(n, rec, B)
            assert (r.state, r.size, r.reserved) == want + (0,), (what, n, r.state, r.size, want)
            assert hb == want[1], (what, n, "the hash kernel would cover other bytes than the frame's")
            seen.add((what.split(" at ")[0], want[0]))
        assert list(d_out) == out
    assert {("all full", CLEAN), ("short last", CLEAN), ("short middle", DELEGATE), ("a failure", DELEGATE), ("a need-history mark", DELEGATE)} <= seen


def test_finish_against_the_host_hash_and_the_content_size_rule():
    L = lib()
    X = fi.lib()
    X.Lizard_XXH32.argtypes = [C.c_char_p, C.c_size_t, C.c_uint]
    X.Lizard_XXH32.restype = C.c_uint
    import random
    rnd = random.Random(9)
    cases = []                                                   # (what, frame, decoded bytes, flags, state before, hash handed in, size, want state)
    for i in range(70):                                          # more than one wave of lanes
        n = COUNTS[i % len(COUNTS)]
        csize = (i >> 1) & 1
        frame = we.raw_frame([1] * n, 1, 1, csize, seed=100 + i)
        rc, info, offs, words, cnt, fb = fi.index(frame)
        assert rc == 0 and cnt == n and fb == len(frame)
        plain = b"".join(frame[o:o + 1] for o in offs)
        h = X.Lizard_XXH32(plain, len(plain), 0)
        kind = i % 7
        flags, before, size, want, hand = DECODE | VERIFY, CLEAN, n, CLEAN, h
        if kind == 1: hand, want = h ^ (1 << rnd.randrange(32)), DELEGATE
        if kind == 2: flags, hand = DECODE, h ^ 1                                    # not verified: a wrong hash is not looked at
        if kind == 3: before, want = DELEGATE, DELEGATE
        if kind == 4: size, want = n + 1, (DELEGATE if csize and n else CLEAN)             # the content-size rule (0 = the header has none)
        if kind == 5: frame, want = frame[:-2] + bytes([frame[-2] ^ 0x10]) + frame[-1:], DELEGATE
        if kind == 6: before, want, flags = DEAD, DEAD, WALK
        cases.append((kind, frame, flags, before, hand, size, want, n if csize else 0))
    frames = [c[1] for c in cases]
    F = len(cases)
    buf, addr = place(frames)
    for seed in SEEDS:
        entries, results, hashes, spans = (Entry * F)(), (Result * F)(), (C.c_uint32 * F)(), (C.c_longlong * (2 * F))()
        for e, r, a, (kind, frame, flags, before, hand, size, want, content), k in zip(entries, results, addr, cases, range(F)):
            e.src, e.srcSize, e.frameBytes, e.contentSize, e.flags = a, len(frame), len(frame), content, flags
            r.size, r.state = (size if before == CLEAN else 0), before
            hashes[k] = hand
        L.emul_unframes_finish(entries, F, hashes, results, spans, seed)
        for k, (r, (kind, frame, flags, before, hand, size, want, content)) in enumerate(zip(results, cases)):
            assert r.state == want, (k, kind, r.state, want)
            assert r.size == (size if want == CLEAN else 0), (k, kind, r.size)
            lo, hi = spans[2 * k], spans[2 * k + 1]
            assert (lo, hi) in ((0, 0), (len(frame) - 4, len(frame))), ("finish read other bytes than the stored checksum", k, lo, hi)
            if kind in (0, 1, 5):
                assert (lo, hi) == (len(frame) - 4, len(frame))
            if kind in (2, 3, 6):
                assert (lo, hi) == (0, 0)
