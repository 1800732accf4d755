"""CPU: LizardGPU_compressFrame_device (lizard_amd/csrc/lizard_frame_device.c) as a unit under test on the fake HIP runtime with
DEFERRED streams (tests/fake_hip.c, tests/pipeline_fake.c as they are, plus tests/frame_device_fake.c: the unit and a plain model of
lz_frame_scan_kernel + lz_frame_gather_kernel).  The block kernels are the oracle.  All chunks of a call are enqueued before the host
waits for anything, on three streams tied by events, so under the lazy and random schedules a missing wait — slots reused before
their gather, a scan before its block kernels, the cursor read back too early — is wrong bytes on every run.  Source and destination
are fake DEVICE allocations with 4 KiB canary margins, uploaded with hipMemcpyAsync on a caller's stream that is NOT synchronised
before the call.  The harness is built with LZC_HASH_PIECE = 40961: the source of a frame is hashed in 10 - 23 pieces through the two
alternating pinned buffers.  Every frame must equal what LizardGPU_compressFrame writes on the same fake, and ok() — no violation,
queues empty at release — follows every call.  The launch the test refuses is the new one (pf_refuse_frame_pack of
tests/frame_device_fake.c: pf_refuse_launch of tests/pipeline_fake.c knows the decoder's launches only).

Wall time, measured on one machine: the whole CPU suite with this module 1291 s (286 tests), this module alone 22 s (21 tests; 9 s of
it build the two forms of the harness, 1 s is the sanitizer program) — so the 265 tests the parent commit has take 1269 s, and this
module is far below the quarter of that which a fake-device module may take.  The oracle stands in for the block kernels and does
100 MB/s and more, which sizes the cases: frames of 3 - 7 blocks of 128 KiB."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_pipeline_fake as pf

HERE = pf.HERE
G = 4096
CANARY = 0xC3
KIB = 1024
BLOCK = 131072
E_GENERIC, E_TOO_SMALL = 1, 11
H2D, D2H = 1, 2
CHUNK_ENV = "LIZARDGPU_FRAME_CHUNK_BLOCKS"
SCHEDULES = pf.SCHEDULES
sched_id = lambda s: "%s%d" % (s[0], s[2])


@functools.lru_cache(maxsize=None)
def built(kind):
    """'lib': the harness with the frame compressor as a shared library; 'asan': tests/frame_device_fake.c's program under
    AddressSanitizer + UBSan.  The emulator's objects (which tests/pipeline_fake.c needs for the decoders) are the plain ones
    test_pipeline_fake builds."""
    return util.build_fake(pf._dir, kind, "frame_device_fake", ("frame_device_fake.c", "pipeline_fake.c", "fake_hip.c"),
                           defines=("-DLZC_HASH_PIECE=40961",))


@functools.lru_cache(maxsize=None)
def harness():
    H = C.CDLL(built("lib"))
    H.fh_set_abort(0)
    H.fh_violations.argtypes = [C.c_char_p, C.c_size_t]
    H.pf_set_chunk_bytes.argtypes = [C.c_size_t]
    H.pf_refuse_frame_pack.argtypes = [C.c_int]
    H.fh_fail_malloc.argtypes = [C.c_int]
    H.LizardGPU_lastError.restype = C.c_char_p
    H.LizardF_isError.argtypes = [C.c_size_t]; H.LizardF_isError.restype = C.c_uint
    H.hipMalloc.argtypes = [C.c_void_p, C.c_size_t]
    H.hipHostMalloc.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipHostFree.argtypes = [C.c_void_p]
    H.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    H.hipStreamCreateWithFlags.argtypes = [C.c_void_p, C.c_uint]
    H.hipStreamSynchronize.argtypes = [C.c_void_p]
    H.LizardGPU_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]; H.LizardGPU_compressFrameBound.restype = C.c_size_t
    H.LizardGPU_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p]; H.LizardGPU_compressFrame.restype = C.c_size_t
    H.LizardGPU_compressFrame_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    H.LizardGPU_compressFrame_device.restype = C.c_size_t
    return H


@functools.lru_cache(maxsize=None)
def caller_stream():
    st = C.c_void_p()
    assert harness().hipStreamCreateWithFlags(C.byref(st), 1) == 0
    return st


def ok(what=""):
    buf = C.create_string_buffer(512)
    n = harness().fh_violations(buf, 512)
    assert n == 0, (what, n, buf.value)


def err_of(r):
    return (1 << 64) - r if harness().LizardF_isError(r) else 0


def schedule(s, chunk_blocks):
    H = harness()
    H.fh_set_schedule(s[1], s[2])
    H.pf_set_chunk_bytes(256 * KIB)                         # two blocks per chunk where the override is unset
    if chunk_blocks is None:
        os.environ.pop(CHUNK_ENV, None)
    else:
        os.environ[CHUNK_ENV] = str(chunk_blocks)


@pytest.fixture(autouse=True)
def _nothing_left_behind():
    yield
    os.environ.pop(CHUNK_ENV, None)
    harness().pf_refuse_frame_pack(0)
    harness().fh_fail_malloc(0)


def cstats():
    out = (C.c_ulonglong * 4)()
    assert harness().LizardGPU_frameCompressDeviceStats(out) == 0
    return list(out)


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
        H = harness()
        H.hipStreamSynchronize(caller_stream())            # (a call refused up front never touched the caller's stream)
        back = C.create_string_buffer(self.size)
        assert H.hipMemcpy(back, self.dev, self.size, D2H) == 0
        raw = back.raw
        assert raw[:G] == bytes([self.fill]) * G and raw[G + self.n:] == bytes([self.fill]) * G, what
        return raw[G:G + self.n]

    def free(self):
        H = harness()
        assert H.hipFree(self.dev) == 0 and H.hipHostFree(self.pin) == 0


def device(data, p, cap, what=None, fail_malloc=0):
    """(error number or 0, frame bytes) of the device entry."""
    H = harness()
    src, dst = Upload(len(data), 0x5A, data), Upload(cap, CANARY)
    if fail_malloc:
        H.hipStreamSynchronize(caller_stream())            # a call that fails before it orders itself behind that stream leaves its work queued, as it may
    H.fh_fail_malloc(fail_malloc)
    r = H.LizardGPU_compressFrame_device(dst.at, cap, src.at, len(data), C.byref(p), caller_stream())
    H.fh_fail_malloc(0)
    ok(("device entry", what, cap))
    body = dst.fetch("the device frame compressor wrote outside d_dst")
    assert src.fetch("the source's margins changed") == bytes(data), "the source changed"
    src.free(); dst.free()
    e = err_of(r)
    if e:
        return e, b""
    assert r <= cap
    return 0, body[:r]


def twin(data, p, cap, what=None):
    H = harness()
    dst = C.create_string_buffer(max(cap, 1))
    r = H.LizardGPU_compressFrame(dst, cap, bytes(data), len(data), C.byref(p))
    ok(("host twin", what, cap))
    e = err_of(r)
    return (e, b"") if e else (0, dst.raw[:r])


def both(data, p, cap=None, what=None):
    cap = harness().LizardGPU_compressFrameBound(len(data), C.byref(p)) if cap is None else cap
    got = device(data, p, cap, what)
    want = twin(data, p, cap, what)
    assert got == want, ("device entry and host twin disagree", what, got[0], want[0], len(got[1]), len(want[1]), cap, harness().LizardGPU_lastError())
    return got


@functools.lru_cache(maxsize=None)
def data():
    d = bytearray(util.datagen(7 * BLOCK, 0.5, 0.0, 97))
    rnd = random.Random(11)
    for lo, hi in ((BLOCK, 2 * BLOCK), (3 * BLOCK + 700, 3 * BLOCK + 9000), (4 * BLOCK, 6 * BLOCK)):      # raw records inside and across chunks
        d[lo:hi] = rnd.randbytes(hi - lo)
    return bytes(d)


@pytest.mark.parametrize("chunk", [1, 2], ids=lambda c: "chunk%d" % c)
@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_frames_of_several_chunks_equal_the_twins(s, chunk):
    H = harness()
    schedule(s, chunk)
    if s[1] == pf.LAZY:
        H.pf_shutdown()                                     # fresh (poisoned) slots and tables under the schedule that runs everything as late as it may
    level = 30 if s[2] in (202, 303) else 10
    for n, checksum, csize in ((3 * BLOCK, 0, 0), (4 * BLOCK + 4321, 1, 1), (5 * BLOCK + 1, 0, 1), (6 * BLOCK, 1, 0), (7 * BLOCK - 1, 1, 1), (7 * BLOCK, 0, 0)):
        plain = data()[:n]
        nb = -(-n // BLOCK)
        p = util.frame_prefs(level, 1, checksum, n if csize else 0, 1)
        s0 = cstats()
        e, frame = both(plain, p, what=(sched_id(s), chunk, n, checksum))
        d = [b - a for a, b in zip(s0, cstats())]
        assert e == 0 and frame == util.compose_frame(plain, level, 1, checksum, csize, util.oracle_compress), (n, e)
        assert d[0] + d[1] == nb and d[2] == -(-nb // chunk) and d[3] == (n if checksum else 0), (n, d)
        if n >= 2 * BLOCK + 1:
            assert d[1] >= 1 and d[0] >= 1, d


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_capacity_degenerate_inputs_and_the_default_chunking(s):
    schedule(s, None)
    plain = data()[:3 * BLOCK + 77]
    p = util.frame_prefs(10, 1, 1, len(plain), 1)
    b = harness().LizardGPU_compressFrameBound(len(plain), C.byref(p))
    s0 = cstats()
    assert both(plain, p, b, "at the bound")[0] == 0
    assert cstats()[2] - s0[2] == 2                         # 256 KiB chunks: two blocks each
    assert both(plain, p, b - 1, "below the bound")[0] == E_TOO_SMALL
    assert both(plain, p, b + 777, "above the bound")[0] == 0
    for checksum in (0, 1):
        assert both(b"", util.frame_prefs(10, 0, checksum, 1, 1), what="empty")[0] == 0
        assert both(b"x", util.frame_prefs(10, 0, checksum, 0, 1), what="one byte")[0] == 0
        # the 1-byte last block under a content-size header: 5 bytes more than the bound counted
        for one in (b"x", data()[BLOCK:2 * BLOCK + 1]):
            q = util.frame_prefs(10, 1, checksum, len(one), 1)
            qb = harness().LizardGPU_compressFrameBound(len(one), C.byref(q))
            assert [both(one, q, qb + k, "1-byte last block")[0] for k in (0, 4, 5)] == [E_TOO_SMALL, E_TOO_SMALL, 0]
    assert both(plain, util.frame_prefs(18, 1, 0, 0, 1), what="level 18")[0] == 5
    assert both(plain, util.frame_prefs(10, 1, 0, 0, 0), what="linked")[0] == 3


@pytest.mark.parametrize("s", SCHEDULES, ids=sched_id)
def test_a_call_that_fails_in_the_machinery_then_a_good_call(s):
    H = harness()
    schedule(s, 1)
    plain = data()[:5 * BLOCK + 9]
    p = util.frame_prefs(10, 1, 1, 0, 1)
    b = H.LizardGPU_compressFrameBound(len(plain), C.byref(p))
    for nth in (1, 2, 4, 6):                                # the first chunk, one whose slots are fresh, one that waits for a gather, the last
        H.pf_refuse_frame_pack(nth)
        got = device(plain, p, b, what=("refused launch", nth))       # ok() inside: nothing left in flight
        assert got == (E_GENERIC, b""), (nth, got[0])
        assert b"refused by the test" in H.LizardGPU_lastError()
        assert both(plain, p, b, "after a refused launch")[0] == 0
    for nth in (1, 2, 3, 6):                                # slots and tables of the three stages
        H.pf_shutdown()
        got = device(plain, p, b, what=("hipMalloc fails", nth), fail_malloc=nth)
        assert got == (E_GENERIC, b""), (nth, got[0])
        assert both(plain, p, b, "after a failed allocation")[0] == 0


def test_core_cases_under_address_sanitizer():
    """tests/frame_device_fake.c's own main: every schedule, 1 / 2 / 4 / unset blocks per chunk, checksum on and off, the capacity
    cases, a refused launch and a failing allocation, with device allocations poisoned while host code runs."""
    try:
        exe = built("asan")
    except subprocess.CalledProcessError:
        pytest.skip("no AddressSanitizer runtime")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "frame_device_fake: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
