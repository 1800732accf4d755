"""CPU: the readers of lizard_amd/csrc/lizard_seek_device.c as a unit under test on the fake HIP runtime with DEFERRED streams:
tests/seek_device_fake.c (the unit; its writer's seams stubbed) linked with tests/unstream_device_fake.c, tests/unframes_device_fake.c,
tests/pipeline_fake.c and tests/fake_hip.c as they are.  LizardGPU_decompressSeekableStream_device must answer what
LizardGPU_decompressStream_device answers on the same fake (ssf_run compares return value, consumed bytes, frame count, decoded count,
decoded bytes and the canary margins) for the sized, mixed and skippable streams of tests/test_stream_decompress_fake_device.py with a
table appended, for every damaged and every lying table, for an intact table over a damaged middle frame, at capacities exact,
exact - 1 and 0 — and LizardGPU_seekDeviceStats must tell the table's path from the fallback.  ok() — no violation of the fake's
rules (async copies into pinned memory only, device memory touched by launches only), queues empty — follows every call."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import seek_inputs as si
import test_pipeline_fake as pf
import test_stream_decompress_fake_device as sd

HERE = pf.HERE
E_TOO_SMALL, E_BLOCK_MODE, E_TYPE, E_SIZE = 11, 3, 13, 14


@functools.lru_cache(maxsize=None)
def built():
    """The harness as a shared library; the emulator's objects are the ones in pf._dir, whichever module built them first."""
    return util.build_fake(pf._dir, "lib", "seek_device_fake",
                           ("seek_device_fake.c", "unstream_device_fake.c", "unframes_device_fake.c", "pipeline_fake.c", "fake_hip.c"),
                           csrc=("lizard_seek_host.c",) + util.FAKE_CSRC, emul=util.FAKE_EMUL + ("unstream_fake_emul.cpp",))


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built())
    H.fh_set_abort(0)
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.ssf_last_error.restype = C.c_char_p
    H.ssf_run.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_void_p]
    H.ssf_items.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    H.ssf_items.restype = C.c_size_t
    H.LizardF_isError.argtypes = [C.c_size_t]; H.LizardF_isError.restype = C.c_uint
    H.fh_set_schedule(pf.LAZY, 1)
    return H


def ok(what=""):
    buf = C.create_string_buffer(512)
    n = harness().fh_violations(buf, 512)
    assert n == 0, (what, n, buf.value)


def err_of(r):
    return (1 << 64) - r if harness().LizardF_isError(r) else 0


def run(stream, cap, flags=0, skew=1, what=None):
    """Both entries on one stream (ssf_run: 0 = one answer); the seekable entry's (result, consumed, frames, decoded, stats growth)."""
    got = (C.c_ulonglong * 8)()
    bad = harness().ssf_run(bytes(stream), len(stream), cap, flags, skew, got)
    ok(what)
    assert bad == 0, (what, bad, harness().ssf_last_error())
    return got[0], got[1], got[2], got[3], list(got[4:8])


def seekable(names):
    """The frames `names` of test_stream_decompress_fake_device.frames() as ITEMS — a skippable frame is the prefix of the frame behind
    it — with their table appended: (stream, decoded total, frames in the stream, items)."""
    f = sd.frames()
    stream, entries, pre = b"", [], b""
    for name in names:
        frame, size = f[name][0], f[name][1]
        if name == "skip":
            pre += frame
            continue
        entries.append((len(stream), size, len(pre), 0))
        stream += pre + frame
        pre = b""
    assert not pre
    return stream + si.pack_table(entries), sum(e[1] for e in entries), len(names) + 1, len(entries)


STREAMS = [("sized frames", ("a", "b", "empty", "c", "one", "raw")), ("a mix: frames without content size", ("b", "n2", "a", "one", "n1", "c")),
           ("a skippable frame as a prefix", ("a", "skip", "b")), ("a linked frame: the batch hands it on, the table stands", ("b", "linked", "one"))]
SMALL = ("b", "skip", "a", "empty", "skip", "n2")                 # four items, two behind a prefix; the last frame without a content size


@pytest.mark.parametrize("s", pf.SCHEDULES[:3], ids=sd.sched_id)
def test_streams_with_a_table_answer_like_the_walk_through_the_table(s):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    for name, names in STREAMS if s[1] != pf.RANDOM else STREAMS[2:3]:
        stream, total, n_frames, _ = seekable(names)
        for cap, flags in ((total, 0), (total + 1000, sd.SKIP_CHECKSUM)):
            r, used, nf, decoded, grown = run(stream, cap, flags, what=(name, cap))
            assert (r, used, nf, decoded) == (total, len(stream), n_frames, total) and H.ssf_last_error() == b"", (name, cap)
            assert grown == [1, 0, 0, 1], (name, cap, grown)
        for cap in (total - 1, 0):
            r, used, nf, decoded, grown = run(stream, cap, what=(name, cap))
            assert err_of(r) == E_TOO_SMALL and grown[:2] == [0, 1], (name, cap, err_of(r), grown)
        # the same frames without a table: the fallback, no table read
        bare = stream[:len(stream) - si.table_bytes(seekable(names)[3])]
        r, used, nf, decoded, grown = run(bare, total, what=(name, "no table"))
        assert (r, used, nf, grown) == (total, len(bare), n_frames - 1, [0, 1, 0, 0]), name
    H.fh_set_schedule(pf.LAZY, 1)


@functools.lru_cache(maxsize=None)
def variants():
    stream, total, n_frames, n = seekable(SMALL)
    return dict(si.damaged(stream) + si.lying(stream))


@pytest.mark.parametrize("name", si.DAMAGED_NAMES + si.LYING_NAMES)
def test_damaged_and_lying_tables_answer_like_the_walk(name):
    stream, total, n_frames, n = seekable(SMALL)
    bad = variants()[name]
    caps = (2 * total,) if name.startswith("two") else (total, total - 1, 0) if name.startswith(("the tag", "entry 1 decodes", "a flag")) else (total,)
    for cap in caps:
        r, used, nf, decoded, grown = run(bad, cap, what=(name, cap))
        assert grown[:2] == [0, 1], (name, cap, grown)
        if cap >= total and not name.startswith(("the size field", "a byte behind", "two")):      # (those three are other streams to the walk)
            assert (r, used, decoded) == (total, len(bad), total), (name, err_of(r))


def test_an_intact_table_over_a_damaged_middle_frame():
    stream, total, n_frames, n = seekable(SMALL)
    entries, _ = si.unpack_table(stream)
    at = entries[1][0] + entries[1][2] + 15 + 4 + 100          # a payload byte of item 1's frame ("a": two blocks, with a checksum)
    f = sd.frames()
    bad = stream[:at] + bytes([stream[at] ^ 0x20]) + stream[at + 1:]
    for cap in (total, total - 1, 0):
        r, used, nf, decoded, grown = run(bad, cap, what=("damaged frame", cap))
        assert grown[:2] == [0, 1], grown
        if cap == total:
            assert err_of(r) and used == entries[1][0] + entries[1][2] and decoded == f["b"][1], (err_of(r), used, decoded)


def items(stream, picks, cap):
    H = harness()
    n = len(picks)
    offs, failed, out = (C.c_uint64 * (n + 1))(), C.c_size_t(99), C.create_string_buffer(max(cap, 1))
    r = H.ssf_items(bytes(stream), len(stream), cap, (C.c_size_t * max(n, 1))(*picks), n, offs, C.byref(failed), out)
    ok(picks)
    return r, failed.value, list(offs), out.raw[:cap]


def test_items_on_the_fake():
    stream, total, n_frames, n = seekable(SMALL)
    entries, _ = si.unpack_table(stream)
    whole = run(stream, total)
    assert whole[0] == total
    sizes = [e[1] for e in entries]
    r, failed, offs, data = items(stream, [0, 3], total)
    assert (r, failed, offs) == (sizes[0] + sizes[3], 99, [0, sizes[0], sizes[0] + sizes[3]])
    r_all, _, _, data_all = items(stream, list(range(n)), total)
    assert r_all == total and data[:sizes[0]] == data_all[:sizes[0]] and data[sizes[0]:r] == data_all[total - sizes[3]:total]
    assert err_of(items(stream, [n], total)[0]) == E_SIZE and err_of(items(stream, [1, 1], total)[0]) == E_BLOCK_MODE
    assert err_of(items(stream[:-si.table_bytes(n)], [0], total)[0]) == E_TYPE
    assert err_of(items(stream, [0, 3], sizes[0] + sizes[3] - 1)[0]) == E_TOO_SMALL
