"""CPU: LizardGPU_decompressStream_device / LizardGPU_streamIndex_device (lizard_amd/csrc/lizard_unstream_device.c) as a unit under test
on the fake HIP runtime with DEFERRED streams: tests/unstream_device_fake.c (the unit, lz_unstream_walk_kernel's real body on the SIMT
emulator through tests/unstream_fake_emul.cpp, and spies on the unit's calls of the batch decoder and of the single-frame entry) linked with
tests/unframes_device_fake.c, tests/pipeline_fake.c and tests/fake_hip.c as they are.  Every stream is a fake DEVICE allocation with
4 KiB canary margins, starting at an odd address, uploaded on a caller's stream that is NOT synchronised before the call; the answer
— return value, consumed bytes, frame count, decoded count, the decoded bytes — must be the LOOP's over
LizardGPU_decompressFrame_device on the same fake (usf_run compares), and the spies' log must show the batches, the capacities and the
hand-over a model written here from the entry's contract expects.  ok() — no violation, queues empty at release — follows every call."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_pipeline_fake as pf
import test_unframe_walk_emul as we
import test_unstream_walk_emul as se

HERE = pf.HERE
SCHEDULES = pf.SCHEDULES
sched_id = lambda s: "%s%d" % (s[0], s[2])
SKIP_CHECKSUM = 1
E_GENERIC, E_TOO_SMALL = 1, 11
GOLDEN = os.path.join(util.GOLDEN_DIR, "frame_ref_linked.liz")
B = 131072


@functools.lru_cache(maxsize=None)
def built(kind):
    """'lib': the harness as a shared library; 'asan': tests/unstream_device_fake.c's program under AddressSanitizer + UBSan.  The
    emulator's objects are the plain ones test_pipeline_fake builds."""
    return util.build_fake(pf._dir, kind, "unstream_device_fake", ("unstream_device_fake.c", "unframes_device_fake.c", "pipeline_fake.c", "fake_hip.c"),
                           emul=util.FAKE_EMUL + ("unstream_fake_emul.cpp",))


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built("lib"))
    H.fh_set_abort(0)
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.usf_last_error.restype = C.c_char_p
    H.usf_refuse.argtypes = [C.c_int]
    H.udf_refuse.argtypes = [C.c_int, C.c_int]
    H.usf_log.argtypes = [C.c_void_p, C.c_size_t]; H.usf_log.restype = C.c_size_t
    H.usf_run.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_void_p]
    H.usf_index.argtypes = [C.c_char_p, C.c_size_t, C.c_uint] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_void_p]
    H.LizardF_isError.argtypes = [C.c_size_t]; H.LizardF_isError.restype = C.c_uint
    return H


def ok(what=""):
    buf = C.create_string_buffer(512)
    n = harness().fh_violations(buf, 512)
    assert n == 0, (what, n, buf.value)


@pytest.fixture(autouse=True)
def _nothing_left_behind():
    os.environ.pop("LIZARDGPU_STREAM_WALK_FRAMES", None)
    yield
    os.environ.pop("LIZARDGPU_STREAM_WALK_FRAMES", None)
    harness().usf_refuse(0)
    for kind in range(4):
        harness().udf_refuse(kind, 0)
    harness().fh_fail_malloc(0)


def run(stream, cap, flags=0, skew=1, fail_malloc=0, want_generic=0, what=None):
    """One stream through usf_run (identity with the loop, margins, source); (result, consumed, frames, decoded, stats growth, log)."""
    H = harness()
    got = (C.c_ulonglong * 8)()
    bad = H.usf_run(bytes(stream), len(stream), cap, flags, skew, fail_malloc, want_generic, got)
    ok(what)
    assert bad == 0, (what, bad, H.usf_last_error())
    raw = (C.c_ulonglong * 8192)()
    n = H.usf_log(raw, 8192)
    assert n <= 8192
    log, i = [], 0
    while i < n:
        if raw[i] == 1:
            k = raw[i + 1]
            log.append(("batch", [tuple(raw[i + 2 + 4 * j:i + 6 + 4 * j]) for j in range(k)], raw[i + 2 + 4 * k]))
            i += 3 + 4 * k
        else:
            assert raw[i] == 2
            log.append(("single", tuple(raw[i + 1:i + 5]), raw[i + 5]))
            i += 6
    return got[0], got[1], got[2], got[3], list(got[4:8]), log


def err_of(r):
    return (1 << 64) - r if harness().LizardF_isError(r) else 0


# ---- streams: (frame bytes, decoded size, what the header promises or None, handed to the single entry unseen) ----
@functools.lru_cache(maxsize=None)
def frames():
    d = util.datagen(3 * B, 0.5, 0.0, 31)
    f = {}
    for name, data, csize, checksum in (("a", d[:B + 5000], 1, 1), ("b", d[7:70007], 1, 0), ("c", d[B:2 * B], 1, 1), ("one", d[99:100], 1, 0),
                                        ("n1", d[5:B + 777], 0, 1), ("n2", d[2 * B:2 * B + 9000], 0, 0)):
        f[name] = (util.compose_frame(data, 10, 1, checksum, csize, util.oracle_compress), len(data), len(data) if csize else None, False)
    f["empty"] = (we.raw_frame([], 1, 1, 0), 0, 0, False)
    f["skip"] = (we.SKIP, 0, 0, False)
    f["raw"] = (we.raw_frame([B, 300], 1, 1, 1, seed=5), B + 300, B + 300, False)
    linked = open(GOLDEN, "rb").read()
    rc, info, _, _, n, fb = fi.index(linked)
    assert rc == 0 and info.blockMode == 0 and n > 1 and fb == len(linked)
    plain = fi.host_one_call(linked, fi.bound(linked))
    assert plain[0] == 0 and plain[2] == len(linked)
    f["linked"] = (linked, len(plain[3]), (info.contentSize or None), True)
    return f


def stream_of(names):
    f = frames()
    return b"".join(f[n][0] for n in names), [f[n] for n in names]


def model(parts, cap, stream_len, flags=0):
    """The log the contract asks for, for a stream of INTACT frames: runs of frames whose size the header gives, every frame but a
    run's last with that size as its capacity, the last with the real remainder; a frame that cannot be settled handed over with
    the loop's arguments.  (log, result or None for an error, consumed, frames, decoded)"""
    log, i, pos, out = [], 0, 0, 0
    offs = [sum(len(p[0]) for p in parts[:k]) for k in range(len(parts))]
    while i < len(parts):
        batch, place, j = [], 0, i
        while j < len(parts) and not parts[j][3]:
            frame, size, known, _ = parts[j]
            last = known is None or known > cap - out - place
            batch.append((offs[j], len(frame), out + place, cap - out - place if last else known))
            j += 1
            if last:
                break
            place += known
        if batch:
            batch[-1] = batch[-1][:3] + (cap - out - sum(b[3] for b in batch[:-1]),)
            log.append(("batch", batch, flags))
        settled = True
        for k, entry in zip(range(i, j), batch):
            if parts[k][1] > entry[3]:
                settled = False
                break
            out += parts[k][1]; pos += len(parts[k][0]); i += 1
        if not settled or (not batch and parts[i][3]):
            log.append(("single", (pos, stream_len - pos, out, cap - out), flags))
            if parts[i][1] > cap - out:
                return log, None, pos, i, out
            out += parts[i][1]; pos += len(parts[i][0]); i += 1
    return log, out, pos, i, out


STREAMS = [("one frame", ("a",)), ("sized frames: one batch", ("a", "b", "empty", "c", "one", "raw")), ("no sizes: a batch each", ("n1", "n2", "n1")),
           ("a mix", ("b", "n2", "a", "one", "n1", "c")), ("a skippable frame in the middle", ("a", "skip", "b")),
           ("the same frame twice", ("b", "b", "n2", "n2")), ("a linked frame between others", ("b", "linked", "c", "one"))]


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_batches_capacities_and_hand_over_follow_the_contract(s):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    if s[1] == pf.LAZY:
        H.pf_shutdown()
    picked = STREAMS if s[1] != pf.RANDOM else STREAMS[s[2] // 101::3]      # (the emulated decoder does 5 MB/s: the random schedules share the streams out)
    for name, names in picked:
        stream, parts = stream_of(names)
        total = sum(p[1] for p in parts)
        first2 = sum(p[1] for p in parts[:2])
        for cap in sorted({total, total - 1, 0, first2, total + 1000}):
            flags = SKIP_CHECKSUM if cap == first2 else 0
            r, used, nf, decoded, grown, log = run(stream, cap, flags, what=(name, cap))
            want_log, want_r, want_used, want_nf, want_out = model(parts, cap, len(stream), flags)
            assert log == want_log, (name, cap, log, want_log)
            assert (used, nf, decoded) == (want_used, want_nf, want_out), (name, cap)
            if want_r is None:
                assert err_of(r) == E_TOO_SMALL and b"dstMaxSize_tooSmall" in H.usf_last_error(), (name, cap, err_of(r))
            else:
                assert r == want_r == decoded and used == len(stream) and H.usf_last_error() == b""
            batches = [e for e in log if e[0] == "batch"]
            singles = [e for e in log if e[0] == "single"]
            settled = nf - sum(1 for e in singles) + (1 if want_r is None else 0)
            assert grown == [settled, len(batches), len(singles), 1], (name, cap, grown)
    stream, parts = stream_of(STREAMS[1][1])
    assert len([e for e in run(stream, sum(p[1] for p in parts))[5] if e[0] == "batch"]) == 1


def test_walk_segments_of_three_frames_over_seven():
    H = harness()
    H.fh_set_schedule(pf.LAZY, 1)
    names = ("b", "one", "skip", "raw", "empty", "n2", "b")
    stream, parts = stream_of(names)
    total = sum(p[1] for p in parts)
    os.environ["LIZARDGPU_STREAM_WALK_FRAMES"] = "3"
    r, used, nf, decoded, grown, log = run(stream, total)
    assert (r, used, nf) == (total, len(stream), 7) and log == model(parts, total, len(stream))[0]
    assert [len(e[1]) for e in log] == [6, 1] and grown == [7, 2, 0, 3], (log, grown)      # the run goes on across two full tables
    os.environ["LIZARDGPU_STREAM_WALK_FRAMES"] = "1"
    assert run(stream, total)[4] == [7, 2, 0, 7]
    os.environ["LIZARDGPU_STREAM_WALK_FRAMES"] = "0"                                  # out of range: the default
    assert run(stream, total)[4] == [7, 2, 0, 1]


def test_null_out_parameters_and_the_empty_stream():
    H = harness()
    H.LizardGPU_decompressStream_device.restype = C.c_size_t
    H.LizardGPU_decompressStream_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    a, b, c = C.c_size_t(7), C.c_size_t(8), C.c_size_t(9)
    assert H.LizardGPU_decompressStream_device(None, 0, None, 0, C.byref(a), C.byref(b), C.byref(c), 0, None) == 0
    assert (a.value, b.value, c.value) == (7, 8, 9), "srcSize == 0 touches nothing"
    assert err_of(H.LizardGPU_decompressStream_device(None, 5, None, 10, C.byref(a), None, None, 0, None)) == E_GENERIC and a.value == 0
    ok()


@pytest.mark.parametrize("case", se.damaged_streams() + [(n, b"".join(se.F()[p] for p in parts), None, 0) for n, parts in (
    ("intact: one frame", ("records",)), ("intact: mixed block size ids", ("bs3", "bs1", "bs7", "bs2", "bs4")), ("intact: an empty frame", ("bs1", "empty", "bs2")),
    ("intact: a skippable frame in the middle", ("bs1", "sized", "skip", "checked", "bs3")),
    ("intact: seven frames", ("bs1", "checked", "skip", "bs4", "empty", "sized", "bs7")))], ids=lambda c: c[0])
def test_the_streams_of_the_walk_test_answer_like_the_loop(case):
    """Every stream of tests/test_unstream_walk_emul.py, intact and damaged, at capacities exact, exact - 1 and 0, with segments of 3."""
    name, stream, ahead, status = case
    H = harness()
    H.fh_set_schedule(pf.RANDOM, 404)
    os.environ["LIZARDGPU_STREAM_WALK_FRAMES"] = "3"
    table, stop, why = se.host_table(stream)
    exact = sum(sum(w & 0x7FFFFFFF for w in fi.index(stream[t[0]:])[3]) for t in table if not t[1] and not t[2][3])      # (raw records: a word is a size)
    for cap in sorted({exact, max(exact - 1, 0), 0}):
        r, used, nf, decoded, grown, log = run(stream, cap, what=(name, cap))
        if status and cap == exact:
            assert err_of(r) == status and used == stop and nf == ahead and decoded == exact, (name, err_of(r), used, nf)
            assert log[-1] == ("single", (stop, len(stream) - stop, exact, 0), 0), (name, log[-1])
        if not status and cap == exact:
            assert (r, used, nf, grown[2]) == (exact, len(stream), len(table), 0), name


def test_stream_index_equals_the_host_index_frame_by_frame():
    H = harness()
    H.fh_set_schedule(pf.RANDOM, 7)
    f = se.F()
    parts = ("bs1", "checked", "skip", "bs4", "empty", "sized", "bs7")
    stream = b"".join(f[p] for p in parts)
    for walk_frames, room in (("3", 16), ("4096", 16), ("2", 4)):
        os.environ["LIZARDGPU_STREAM_WALK_FRAMES"] = walk_frames
        offs, fb, infos, nrec = (C.c_uint64 * room)(), (C.c_uint64 * room)(), (util.FrameInfo * room)(), (C.c_size_t * room)()
        n, total = C.c_size_t(99), C.c_size_t(99)
        assert H.usf_index(stream, len(stream), 3, offs, fb, infos, nrec, room, C.byref(n), C.byref(total)) == 0
        ok()
        assert (n.value, total.value) == (7, len(stream))
        pos = 0
        for k, p in enumerate(parts[:room]):
            rc, info, _, _, cnt, fbytes = fi.index(f[p])
            assert (offs[k], fb[k], nrec[k]) == (pos, fbytes, cnt), (k, p)
            assert bytes(infos[k]) == bytes(info), (k, p)
            pos += fbytes
    # a refused frame: its code, the frames in front of it, its offset; arrays may be NULL
    for name, bad, ahead, status in se.damaged_streams():
        n, total = C.c_size_t(99), C.c_size_t(99)
        assert H.usf_index(bad, len(bad), 0, None, None, None, None, 0, C.byref(n), C.byref(total)) == -status, name
        ok()
        assert (n.value, total.value) == (ahead, se.host_table(bad)[1]), name
        assert b"refused" in H.usf_last_error()


@pytest.mark.parametrize("s", SCHEDULES[:3], ids=sched_id)
def test_a_call_that_fails_in_the_machinery_then_a_good_call(s):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    stream, parts = stream_of(("b", "n2", "one"))
    total = sum(p[1] for p in parts)
    H.usf_refuse(1)
    r = run(stream, total, want_generic=1, what="refused stream walk")
    assert err_of(r[0]) == E_GENERIC and r[1:4] == (0, 0, 0) and b"refused by the test" in H.usf_last_error()
    for kind in range(4):                                   # a launch of the batch decoder: the second batch fails, the first one's frames stand
        H.udf_refuse(kind, 2 if kind == 0 else 1)
        r = run(stream, total, want_generic=1, what=("refused batch launch", kind))
        assert err_of(r[0]) == E_GENERIC and b"refused by the test" in H.usf_last_error()
        if kind == 0:
            H.udf_refuse(0, 3)                              # (walk launches: count and fill of the first batch, then the second batch's count)
            r = run(stream, total, want_generic=1)
            assert r[1:4] == (len(parts[0][0]) + len(parts[1][0]), 2, parts[0][1] + parts[1][1])
    run(stream, total, what="after refused launches")
    H.pf_shutdown()                                         # fresh context: the first device allocation of the call is the walk's table
    r = run(stream, total, fail_malloc=1, want_generic=1, what="hipMalloc fails")
    assert err_of(r[0]) == E_GENERIC and r[1:4] == (0, 0, 0)
    run(stream, total, what="after a failed allocation")


def test_core_cases_under_address_sanitizer():
    """tests/unstream_device_fake.c's own main as a stand-alone program under AddressSanitizer + UBSan: four schedules, levels 10 and 30,
    a one-batch stream with segments of 2 and of 4 096 frames, capacities exact, one short, the first two frames and 0, truncated
    streams, a mixed stream with the reference's linked frame, garbage at the end, a refused launch of each kind and a failing
    allocation, with device allocations poisoned while host code runs."""
    if not util.sanitizer_runtime(pf._dir):
        pytest.skip("no AddressSanitizer runtime: a trivial program does not build with -fsanitize=address,undefined")
    exe = built("asan")                                     # (a failure of THIS build fails the test)
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "unstream_device_fake: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
