"""CPU: LizardGPU_decompressFrames_device (lizard_amd/csrc/lizard_unframes_device.c) as a unit under test on the fake HIP runtime with
DEFERRED streams (tests/fake_hip.c, tests/pipeline_fake.c as they are, plus tests/unframes_device_fake.c: the unit and plain sequential
models of its four launches and of lz_xxh32_frames_kernel; records decode through the emulator's objects, the walk is the real one).
Everything behind the count pass is enqueued before the host waits again, so under the lazy and random schedules a missing order — the
decode before the tables are filled, the hash before the settle, the result records read back too early — is wrong answers on every
run.  udf_cases of the harness builds the standard batch (128 KiB blocks, frames of 0 - 3 blocks, 14 block records in the batch part):
clean frames with checksum and content size on and off, a frame one byte short of capacity, a flushed frame and
tests/golden/frame_ref_linked.liz among them (both delegated), frames cut in the header and in the chain, a corrupt block, a wrong
checksum with and without the skip flag, a skippable frame, a null entry.  Every source and destination is a fake DEVICE allocation
with 4 KiB canary margins, uploaded on a caller's stream that is NOT synchronised before the call; every frame's result, consumed count
and bytes must equal LizardGPU_decompressFrame_device's on the same fake for the same bytes and capacity.  ok() — no violation, queues
empty at release — follows every call.

Wall time of the module: 32 s measured, 13 s of it the sanitizer program and its build (the emulator decodes every block twice, once
per entry, where the sibling test_frames_compress_fake_device, 9 s, has the oracle for its block kernels)."""
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
SCHEDULES = pf.SCHEDULES
sched_id = lambda s: "%s%d" % (s[0], s[2])
ERR_HIP, ERR_NOMEM = 4, 5
SKIP_CHECKSUM = 1
WALK, DECODE, SETTLE, FINISH = range(4)
GOLDEN = os.path.join(util.GOLDEN_DIR, "frame_ref_linked.liz").encode()


@functools.lru_cache(maxsize=None)
def built(kind):
    """'lib': the harness with the batch decoder as a shared library; 'asan': tests/unframes_device_fake.c's program under
    AddressSanitizer + UBSan.  The emulator's objects are the plain ones test_pipeline_fake builds."""
    return util.build_fake(pf._dir, kind, "unframes_device_fake", ("unframes_device_fake.c", "pipeline_fake.c", "fake_hip.c"))


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built("lib"))
    H.fh_set_abort(0)
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.udf_refuse.argtypes = [C.c_int, C.c_int]
    H.udf_last_error.restype = C.c_char_p
    H.udf_cases.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return H


def ok(what=""):
    buf = C.create_string_buffer(512)
    n = harness().fh_violations(buf, 512)
    assert n == 0, (what, n, buf.value)


@pytest.fixture(autouse=True)
def _nothing_left_behind():
    yield
    for kind in range(4):
        harness().udf_refuse(kind, 0)
    harness().fh_fail_malloc(0)


def cases(level=10, checksum=0, csize=0, flags=0, golden=None, null=-1, fail_malloc=0, want_rc=0, what=None):
    """The standard batch through udf_cases (every frame against the single-frame entry, margins, sources); the growth of the statistics."""
    H = harness()
    grown = (C.c_ulonglong * 4)()
    bad = H.udf_cases(level, checksum, csize, flags, golden, null, fail_malloc, want_rc, grown)
    ok(what)
    assert bad == 0, (what, H.udf_last_error())
    return list(grown)


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_every_frame_of_a_batch_equals_the_single_entrys(s):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    if s[1] == pf.LAZY:
        H.pf_shutdown()                                     # fresh (poisoned) tables under the schedule that runs everything as late as it may
    level = 30 if s[2] in (202, 303) else 10
    checksum, csize = (s[2] & 1) ^ 1, s[2] >> 1 & 1
    d = cases(level, checksum, csize, 0, GOLDEN, what=(sched_id(s), checksum, csize))
    # handed on: one byte short, flushed, linked, the corrupt block, the 1-byte block in a 1-byte buffer (lz_unframe_record refuses a
    # record longer than its room: the single entry decodes it in a staging slot), and the wrong checksum where there is one;
    # settled: 3, 1 and 0 blocks, and the frame whose checksum would be wrong where there is none
    assert d[3] == 1 and d[2] == 5 + checksum and d[1] == 3 + (1 - checksum) and d[0] == 11 + 10, d
    assert b"frame 3 refused: ERROR_dstMaxSize_tooSmall" in H.udf_last_error()
    d = cases(level, 1 - checksum, 1 - csize, 0, None, what=(sched_id(s), "the other half"))
    assert d[3] == 1 and d[2] == 4 + (1 - checksum) and d[1] + d[2] == 8, d
    # the skip flag: the wrong checksum is not looked at, on the device or by the single entry; a null entry among the others
    d = cases(level, 1, csize, SKIP_CHECKSUM, None, null=1, what=(sched_id(s), "skip flag, null entry"))
    assert d[1] + d[2] == 7 and d[1] >= 3 and d[2] >= 3, d      # (the corrupt block may decode to a block of other bytes: nothing looks at them then)
    assert b"frame 1 refused" in H.udf_last_error()


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_a_call_that_fails_in_the_machinery_then_a_good_call(s):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    for kind, nth in ((WALK, 1), (WALK, 2), (DECODE, 1), (SETTLE, 1), (FINISH, 1)):      # the count pass, then each launch of the fill pass
        H.udf_refuse(kind, nth)
        cases(10, 1, 0, want_rc=-ERR_HIP, what=("refused launch", kind, nth))      # ok() inside: nothing left in flight
        assert b"refused by the test" in H.udf_last_error()
    cases(10, 1, 0, what="after refused launches")
    for nth in (1, 2):                                      # the tables of the count pass, the tables of the fill pass
        H.pf_shutdown()
        cases(10, 1, 0, fail_malloc=nth, want_rc=-ERR_NOMEM, what=("hipMalloc fails", nth))
        cases(10, 1, 0, what="after a failed allocation")


def test_core_cases_under_address_sanitizer():
    """tests/unframes_device_fake.c's own main as a program of its own: four schedules, levels 10 and 30, checksum on and off, the skip
    flag, a null entry, a refused launch of each kind and a failing allocation, with device allocations poisoned while host code runs."""
    try:
        exe = built("asan")
    except subprocess.CalledProcessError:
        pytest.skip("no AddressSanitizer runtime")
    r = subprocess.run([exe, GOLDEN.decode()], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "unframes_device_fake: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
