"""CPU: LizardGPU_compressFrames_device (lizard_amd/csrc/lizard_frames_device.c) as a unit under test on the fake HIP runtime with
DEFERRED streams (tests/fake_hip.c, tests/pipeline_fake.c as they are, plus tests/frames_device_fake.c: the unit and plain sequential
models of lz_frames_scan_kernel + lz_frames_gather_kernel, lz_xxh32_frames_kernel and lz_frames_finish_kernel).  The block kernels are
the oracle over a ragged batch.  All chunks of a batch, the hash and the finish are enqueued before the host waits for anything, on
three streams tied by events, so under the lazy and random schedules a missing wait — slots reused before their gather, a scan before
its block kernels or before the tables are uploaded, the finish before the hash, the result records read back too early — is wrong
bytes on every run.  fdf_batch of the harness runs one batch: every source and destination is a fake DEVICE allocation with 4 KiB
canary margins, uploaded with hipMemcpyAsync on a caller's stream that is NOT synchronised before the call, sources at byte offsets
0 - 3; every results[i] and every frame must equal what LizardGPU_compressFrame writes for that buffer on the same fake; a frame refused
below its bound must leave its region untouched.  ok() — no violation, queues empty at release — follows every call.

The oracle stands in for the block kernels, which sizes the cases: frames of 0 - 5 blocks of 128 KiB, 14 blocks per batch."""
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
SCHEDULES = pf.SCHEDULES
sched_id = lambda s: "%s%d" % (s[0], s[2])
ERR_HIP, ERR_NOMEM = 4, 5
# (offset into the harness's data, bytes): 3, 1, 0, 2 and 5 blocks, one byte, one block and a byte (behind a block of noise)
FRAMES = [(0, 3 * BLOCK), (3 * BLOCK, BLOCK), (0, 0), (4 * BLOCK, 2 * BLOCK), (6 * BLOCK, 5 * BLOCK), (777, 1), (9 * BLOCK - 1, BLOCK + 1)]
TOTAL_BLOCKS = 14


@functools.lru_cache(maxsize=None)
def built(kind):
    """'lib': the harness with the batch compressor as a shared library; 'asan': tests/frames_device_fake.c's program under
    AddressSanitizer + UBSan.  The emulator's objects (which tests/pipeline_fake.c needs for the decoders) are the plain ones
    test_pipeline_fake builds."""
    return util.build_fake(pf._dir, kind, "frames_device_fake", ("frames_device_fake.c", "pipeline_fake.c", "fake_hip.c"))


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built("lib"))
    H.fh_set_abort(0)
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.pf_set_chunk_bytes.argtypes = [C.c_size_t]
    H.pf_refuse_frames_pack.argtypes = [C.c_int]
    H.fdf_last_error.restype = C.c_char_p
    H.fdf_batch.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
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
    harness().pf_refuse_frames_pack(0)
    harness().fh_fail_malloc(0)


def batch(frames, level=10, checksum=0, csize=0, cap_deltas=None, fail_malloc=0, want_rc=0, what=None):
    """One batch through fdf_batch (every frame against the host twin, margins, sources); the growth of the statistics."""
    H = harness()
    n = len(frames)
    offs = (C.c_size_t * n)(*[f[0] for f in frames])
    sizes = (C.c_size_t * n)(*[f[1] for f in frames])
    deltas = (C.c_long * n)(*(cap_deltas or [0] * n))
    grown = (C.c_ulonglong * 4)()
    bad = H.fdf_batch(n, offs, sizes, deltas, level, 1, checksum, csize, fail_malloc, want_rc, grown)
    ok(what)
    assert bad == 0, (what, H.fdf_last_error())
    return list(grown)


@pytest.mark.parametrize("chunk", [1, 2, 4, None], ids=lambda c: "chunk%s" % c)
@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_every_frame_of_a_batch_equals_the_twins(s, chunk):
    """Chunk borders inside frames, between frames, and chunks that hold several whole frames; checksum and content size on and off."""
    H = harness()
    schedule(s, chunk)
    if s[1] == pf.LAZY:
        H.pf_shutdown()                                     # fresh (poisoned) slots and tables under the schedule that runs everything as late as it may
    level = 30 if s[2] in (202, 303) else 10
    per = 2 if chunk is None else chunk
    for checksum, csize in ((0, 0), (1, 1)) if chunk in (1, None) else ((1, 0), (0, 1)):
        d = batch(FRAMES, level, checksum, csize, what=(sched_id(s), chunk, checksum, csize))
        # with a content size the 1-byte frame answers dstMaxSize_tooSmall at its bound, as the twin does: its block is in no count
        assert d[0] + d[1] == TOTAL_BLOCKS if not csize else TOTAL_BLOCKS - 3 <= d[0] + d[1] < TOTAL_BLOCKS, d
        assert d[1] >= 2 and d[0] >= 8, d
        assert d[2] == -(-TOTAL_BLOCKS // per) and d[3] == 0, d


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_refused_frames_do_not_stop_their_neighbours(s):
    schedule(s, 2)
    # one frame one byte below its bound between two good ones (one of them with room to spare): refused, its region untouched
    d = batch(FRAMES, 10, 1, 0, cap_deltas=[0, 77, 0, -1, 0, 0, 0], what="one below its bound")
    assert d[0] + d[1] == TOTAL_BLOCKS - 2 and d[2] == (TOTAL_BLOCKS - 2) // 2, d
    assert b"frame 3 refused: ERROR_dstMaxSize_tooSmall" in harness().fdf_last_error()
    # level 18: every frame answers compressionLevel_invalid, nothing is launched
    assert batch(FRAMES, 18, 0, 0, what="level 18") == [0, 0, 0, 0]


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_a_call_that_fails_in_the_machinery_then_a_good_call(s):
    H = harness()
    schedule(s, 1)
    frames = FRAMES[:5]
    for nth in (1, 2, 4, 11):                               # the first chunk, one whose slots are fresh, one that waits for a gather, the last
        H.pf_refuse_frames_pack(nth)
        batch(frames, 10, 1, 0, want_rc=-ERR_HIP, what=("refused launch", nth))      # ok() inside: nothing left in flight
        assert b"refused by the test" in H.fdf_last_error()
        batch(frames, 10, 1, 0, what="after a refused launch")
    for nth in (1, 2, 3, 7):                                # the tables, then slots and tables of the three stages
        H.pf_shutdown()
        batch(frames, 10, 1, 0, fail_malloc=nth, want_rc=-ERR_NOMEM, what=("hipMalloc fails", nth))
        batch(frames, 10, 1, 0, what="after a failed allocation")


def test_core_cases_under_address_sanitizer():
    """tests/frames_device_fake.c's own main: every schedule, 1 / 2 / 4 / unset blocks per chunk, checksum on and off, levels 10 and 30,
    a frame below its bound, level 18, a refused launch and a failing allocation, with device allocations poisoned while host code
    runs."""
    try:
        exe = built("asan")
    except subprocess.CalledProcessError:
        pytest.skip("no AddressSanitizer runtime")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "frames_device_fake: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
