"""CPU: LizardGPU_compressStream_device (lizard_amd/csrc/lizard_stream_device.c) as a unit under test on the fake HIP runtime with
DEFERRED streams (tests/fake_hip.c, tests/pipeline_fake.c as they are, plus tests/stream_device_fake.c: the unit and plain sequential
models of lz_stream_scan_kernel + lz_frames_gather_kernel, lz_xxh32_frames_kernel and lz_stream_finish_kernel).  The block kernels are
the oracle over a ragged batch.  All chunks of a call, the hash and the finish are enqueued before the host waits for anything, on
three streams tied by events, so under the lazy and random schedules a missing wait — slots reused before their gather, a scan before
its block kernels or before the tables are uploaded, the finish before the hash, the result read back too early — is wrong bytes on
every run.  sdf_batch of the harness runs one call: every source and the destination is a fake DEVICE allocation with 4 KiB canary
margins, uploaded with hipMemcpyAsync on a caller's stream that is NOT synchronised before the call, sources at byte offsets 0 - 3;
the stream must equal prefix + LizardGPU_compressFrame's frame (at its bound + 8) per frame on the same fake, the frame offsets must
be right, and LizardF_decompress (lizard_frame_host.c) must read every [offset i, offset i + 1) back: the prefix, a skippable frame
as a tensor header is one, stepped over and the frame decoded to the source.  ok() — no violation, queues empty at release — follows
every call.

The oracle stands in for the block kernels, which sizes the cases: frames of 0 - 5 blocks of 128 KiB, 14 blocks per call."""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_pipeline_fake as pf

HERE = pf.HERE
BLOCK = 131072
CHUNK_ENV = "LIZARDGPU_FRAME_CHUNK_BLOCKS"
SCHEDULES = [s for s in pf.SCHEDULES if s[1] != pf.EAGER]   # lazy, and three seeds of random
sched_id = lambda s: "%s%d" % (s[0], s[2])
E_GENERIC, E_BLOCK_MODE, E_LEVEL, E_TOO_SMALL = 1, 3, 5, 11
CAP_BOUND, CAP_EXACT, CAP_ONE_BELOW = 0, 1, 2
# (offset into the harness's data, bytes): the frames of test_frames_compress_fake_device — 3, 1, 0, 2 and 5 blocks, one byte, one
# block and a byte (behind a block of noise, so the 1-byte block makes the 10-byte record) — with a second empty frame next to the
# first and an empty frame at the end
FRAMES = [(0, 3 * BLOCK), (3 * BLOCK, BLOCK), (0, 0), (0, 0), (4 * BLOCK, 2 * BLOCK), (6 * BLOCK, 5 * BLOCK), (777, 1), (9 * BLOCK - 1, BLOCK + 1), (0, 0)]
TOTAL_BLOCKS = 14
HEADERS = [56, 0, 48, 64, 8, 56, 72, 56, 48]               # prefixes that are skippable frames (or absent)


def err(code):
    return (1 << 64) - code


@functools.lru_cache(maxsize=None)
def built(kind):
    """'lib': the harness with the stream compressor as a shared library; 'asan': tests/stream_device_fake.c's program under
    AddressSanitizer + UBSan.  The emulator's objects (which tests/pipeline_fake.c needs for the decoders) are the plain ones
    test_pipeline_fake builds."""
    return util.build_fake(pf._dir, kind, "stream_device_fake", ("stream_device_fake.c", "pipeline_fake.c", "fake_hip.c"))


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built("lib"))
    H.fh_set_abort(0)
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.pf_set_chunk_bytes.argtypes = [C.c_size_t]
    H.sdf_refuse_pack.argtypes = [C.c_int]
    H.sdf_last_error.restype = C.c_char_p
    H.sdf_batch.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_size_t,
                            C.c_long, C.c_void_p]
    return H


def ok(what=""):
    buf = C.create_string_buffer(512)
    n = harness().fh_violations(buf, 512)
    assert n == 0, (what, n, buf.value)


def schedule(s, chunk_blocks):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    H.pf_set_chunk_bytes(256 * 1024)                        # two blocks per chunk where the override is unset
    if chunk_blocks is None:
        os.environ.pop(CHUNK_ENV, None)
    else:
        os.environ[CHUNK_ENV] = str(chunk_blocks)


@pytest.fixture(autouse=True)
def _nothing_left_behind():
    yield
    os.environ.pop(CHUNK_ENV, None)
    harness().sdf_refuse_pack(0)
    harness().fh_fail_malloc(0)


def call(frames, prefixes=None, level=10, checksum=0, cap=CAP_BOUND, independent=1, null_sources=(), fail_malloc=0, want=0, failed=-1, what=None):
    """One call through sdf_batch (the stream against prefix + twin, offsets, LizardF_decompress, margins, sources); the growth of
    LizardGPU_streamCompressDeviceStats and, behind it, of LizardGPU_frameCompressDeviceStats."""
    H = harness()
    n = len(frames)
    offs = (C.c_size_t * n)(*[f[0] for f in frames])
    sizes = (C.c_size_t * n)(*[f[1] for f in frames])
    pre = (C.c_size_t * n)(*prefixes[:n]) if prefixes is not None else None
    grown = (C.c_ulonglong * 8)()
    mask = sum(1 << i for i in null_sources)
    bad = H.sdf_batch(n, offs, sizes, pre, level, 1, independent, checksum, cap, mask, fail_malloc, err(want) if want else 0, failed, grown)
    ok(what)
    assert bad == 0, (what, H.sdf_last_error())
    return list(grown)


@pytest.mark.parametrize("chunk", [1, 2, 3, None], ids=lambda c: "chunk%s" % c)
@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_the_stream_is_prefix_and_twin_frame_back_to_back(s, chunk):
    """Chunk borders inside frames, between frames and on empty frames; checksum on and off; with tensor-header-like prefixes, without
    any, and with prefixes of one byte."""
    H = harness()
    schedule(s, chunk)
    if s[1] == pf.LAZY:
        H.pf_shutdown()                                     # fresh (poisoned) slots and tables under the schedule that runs everything as late as it may
    level = 30 if s[2] in (202, 303) else 10
    per = 2 if chunk is None else chunk
    for checksum, prefixes in ((0, HEADERS), (1, None)) if chunk in (1, None) else ((1, HEADERS), (0, [1] * len(FRAMES))):
        d = call(FRAMES, prefixes, level, checksum, what=(sched_id(s), chunk, checksum, prefixes))
        assert d[0] == len(FRAMES) and d[1] >= 2, d
        assert d[2] == -(-TOTAL_BLOCKS // per) and d[3] == 1, d
        assert d[4:] == [0, 0, 0, 0], ("LizardGPU_frameCompressDeviceStats moved", d)


@pytest.mark.parametrize("s", SCHEDULES[:2], ids=sched_id)
def test_capacity_exact_one_below_and_the_bound(s):
    schedule(s, 3)
    for checksum in (0, 1):
        call(FRAMES, HEADERS, 10, checksum, cap=CAP_EXACT, what="exact")
        d = call(FRAMES, HEADERS, 10, checksum, cap=CAP_ONE_BELOW, want=E_TOO_SMALL, what="one below")     # (margins checked inside)
        assert d[0] == 0 and d[3] == 1, d
        call(FRAMES, HEADERS, 10, checksum, cap=CAP_BOUND, what="bound")
    # the frames whose own bound is 5 bytes short (one byte; a block and a byte behind noise), alone and together, at the bound
    for frames in ([FRAMES[6]], [FRAMES[7]], [FRAMES[6], FRAMES[7], FRAMES[6]], [FRAMES[8]]):
        call(frames, None, 10, 1, cap=CAP_BOUND, what=("bound", frames))
        call(frames, None, 10, 1, cap=CAP_EXACT, what=("exact", frames))
        call(frames, None, 10, 1, cap=CAP_ONE_BELOW, want=E_TOO_SMALL, what=("one below", frames))


@pytest.mark.parametrize("s", SCHEDULES[:2], ids=sched_id)
def test_a_frame_refused_up_front_stops_the_call_before_any_launch(s):
    schedule(s, 2)
    # level 23 has no kernel: frame 0 decides
    assert call(FRAMES, HEADERS, 23, 0, want=E_LEVEL, failed=0, what="level 23")[:4] == [0, 0, 0, 0]
    assert b"frame 0 refused: ERROR_compressionLevel_invalid" in harness().sdf_last_error()
    # linked mode: a frame of up to one block is written independent, the first of two blocks is refused; the later one of five changes nothing
    late = [FRAMES[1], FRAMES[2], FRAMES[4], FRAMES[5]]
    assert call(late, HEADERS, 10, 1, independent=0, want=E_BLOCK_MODE, failed=2, what="linked")[:4] == [0, 0, 0, 0]
    assert call(late[:2], HEADERS, 10, 1, independent=0, what="linked, one block at most")[0] == 2
    # a null source with a size; a second one behind it, and an empty frame with a null source in front of it, change nothing
    assert call(FRAMES, HEADERS, 10, 0, null_sources=(2, 4, 7), want=E_GENERIC, failed=4, what="null source")[:4] == [0, 0, 0, 0]
    assert b"frame 4 refused" in harness().sdf_last_error()
    # and a later refusable frame of another kind does not change the index either: linked, frame 0 (three blocks) in front of the null source
    assert call(FRAMES, HEADERS, 10, 0, independent=0, null_sources=(1,), want=E_BLOCK_MODE, failed=0, what="two kinds")[:4] == [0, 0, 0, 0]


@pytest.mark.parametrize("s", SCHEDULES[:3], ids=sched_id)
def test_a_call_that_fails_in_the_machinery_then_a_good_call(s):
    H = harness()
    schedule(s, 1)
    frames = FRAMES[:6]                                     # 11 blocks
    for nth in (1, 2, 4, 11):                               # the first chunk, one whose slots are fresh, one that waits for a gather, the last
        H.sdf_refuse_pack(nth)
        call(frames, HEADERS, 10, 1, want=E_GENERIC, what=("refused launch", nth))       # ok() inside: nothing left in flight
        assert b"refused by the test" in H.sdf_last_error()
        call(frames, HEADERS, 10, 1, what="after a refused launch")
    for nth in (1, 2, 3, 7):                                # the tables, then slots and tables of the three stages
        H.pf_shutdown()
        call(frames, HEADERS, 10, 1, fail_malloc=nth, want=E_GENERIC, what=("hipMalloc fails", nth))
        call(frames, HEADERS, 10, 1, what="after a failed allocation")


def test_no_frames_and_null_arrays():
    H = harness()
    H.LizardGPU_compressStream_device.restype = C.c_size_t
    H.LizardGPU_compressStream_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t] + [C.c_void_p] * 8
    H.LizardGPU_compressStreamBound.restype = C.c_size_t
    H.LizardGPU_compressStreamBound.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    H.LizardGPU_compressFrameBound.restype = C.c_size_t
    H.LizardGPU_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
    one = (C.c_size_t * 1)(5)
    ptr = (C.c_void_p * 1)(4096)
    assert H.LizardGPU_compressStream_device(None, 0, 0, None, None, None, None, None, None, None, None) == 0
    assert H.LizardGPU_compressStream_device(4096, 100, 1, None, one, None, None, None, None, None, None) == err(E_GENERIC)
    assert H.LizardGPU_compressStream_device(4096, 100, 1, ptr, None, None, None, None, None, None, None) == err(E_GENERIC)
    assert H.LizardGPU_compressStream_device(None, 100, 1, ptr, one, None, None, None, None, None, None) == err(E_GENERIC)
    assert H.LizardGPU_compressStream_device(4096, 100, 1, ptr, one, None, one, None, None, None, None) == err(E_GENERIC)
    ok("null arrays")
    sizes = (C.c_size_t * 3)(0, 1, 3 * BLOCK + 1)
    pre = (C.c_size_t * 3)(56, 0, 9)
    want = sum(H.LizardGPU_compressFrameBound(s, None) + 8 for s in sizes)
    assert H.LizardGPU_compressStreamBound(3, sizes, None, None) == want
    assert H.LizardGPU_compressStreamBound(3, sizes, pre, None) == want + 65
    assert H.LizardGPU_compressStreamBound(0, None, None, None) == 0


def test_one_pass_under_address_sanitizer():
    """tests/stream_device_fake.c's own main: the batch under three schedules with 1 / unset / 3 blocks per chunk, checksum on and off,
    the three capacities, the up-front refusals, a refused launch and a failing allocation, with device allocations poisoned while host
    code runs."""
    try:
        exe = built("asan")
    except subprocess.CalledProcessError:
        pytest.skip("no AddressSanitizer runtime")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "stream_device_fake: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
