"""LizardGPU_compressFrame_device: data that lies in device memory compressed into a Lizard frame in device memory.  Every case also
runs the host-memory twin LizardGPU_compressFrame on the same bytes with the same preferences and capacity and requires the same
return value and the same frame bytes; where oracle/_ref holds the compiled reference the frame is also compared with its
LizardF_compressFrame, otherwise with util.compose_frame over the oracle's block compressor.  Source and destination are torch
tensors with 4 KiB canary margins on both sides, checked after every call."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_frame_decompress_gpu as fd
import test_frame_decompress_device as dd

pytestmark = pytest.mark.gpu

G = dd.G
CANARY = dd.CANARY
E_GENERIC, E_BLOCK_SIZE, E_BLOCK_MODE, E_LEVEL, E_TOO_SMALL, E_FRAME_TYPE = 1, 2, 3, 5, 11, 13
BS = util.FRAME_BLOCK_SIZES
BLOCK = 128 << 10
CHUNK_ENV = "LIZARDGPU_FRAME_CHUNK_BLOCKS"


def lib():
    return dd.lib()


def cstats():
    out = (C.c_ulonglong * 4)()
    assert lib().LizardGPU_frameCompressDeviceStats(out) == 0
    return list(out)


def grown(s0):
    return [b - a for a, b in zip(s0, cstats())]


@pytest.fixture(autouse=True)
def _no_chunk_override_left_behind():
    yield
    os.environ.pop(CHUNK_ENV, None)


def set_chunk(blocks):
    if blocks is None:
        os.environ.pop(CHUNK_ENV, None)
    else:
        os.environ[CHUNK_ENV] = str(blocks)


def bound_of(n, p):
    return lib().LizardGPU_compressFrameBound(n, C.byref(p))


def device(data, p, cap):
    """(error number or 0, bytes) of the device entry on torch's current stream; the margins of both tensors checked."""
    import torch
    L = lib()
    src, dst = dd.padded(data, 0x5A), dd.padded(bytes(cap), CANARY)
    dst[G:G + cap] = CANARY
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = L.LizardGPU_compressFrame_device(dst.data_ptr() + G, cap, src.data_ptr() + G, len(data), C.byref(p), stream)
    body = dd.margins_intact(dst, cap, CANARY, "the device frame compressor wrote outside d_dst")
    assert dd.margins_intact(src, len(data), 0x5A, "the source's margins changed").tobytes() == bytes(data), "the source changed"
    e = fi.err_of(r)
    if e:
        return e, body.tobytes()
    assert r <= cap
    return 0, body[:r].tobytes()


@functools.lru_cache(maxsize=None)
def _twin(data, prefs, cap):
    L = lib()
    p = util.FramePrefs.from_buffer_copy(prefs)
    dst = C.create_string_buffer(max(cap, 1))
    src = C.create_string_buffer(data, max(len(data), 1))
    r = L.LizardGPU_compressFrame(dst, cap, src, len(data), C.byref(p))
    e = fi.err_of(r)
    return (e, b"") if e else (0, dst.raw[:r])


def twin(data, p, cap):
    """(error number or 0, bytes) of LizardGPU_compressFrame; computed once for the same bytes, preferences and capacity (the blocks
    per chunk of the device entry are nothing the twin knows of)."""
    return _twin(bytes(data), bytes(p), cap)


def both(data, p, cap=None, what=None):
    """The device entry and the host twin: the same return value, the same frame; returned once."""
    cap = bound_of(len(data), p) if cap is None else cap
    e, got = device(data, p, cap)
    te, want = twin(data, p, cap)
    assert e == te, ("device entry and host twin disagree", what, e, te, cap, len(data), lib().LizardGPU_lastError())
    if not e:
        assert got == want, ("the frames differ", what, len(got), len(want), cap)
    return e, got


@functools.lru_cache(maxsize=None)
def oracle_block(block, level):
    return util.oracle_compress(block, level)


@functools.lru_cache(maxsize=None)
def expected_frame(data, level, bsid, checksum, csize):
    """The reference's frame where it is compiled, else the restatement of its frame layer over the oracle's blocks."""
    ref = util.reference_frame(data, util.frame_prefs(level, bsid, checksum, len(data) if csize else 0, 1))
    return ref if ref is not None else util.compose_frame(data, level, bsid, checksum, csize, oracle_block)


@functools.lru_cache(maxsize=None)
def mixed(n_bytes):
    """P50 with runs of noise from a fixed seed: whole blocks (1, 4, 5, 8) and stretches inside blocks, so that raw and compressed
    records alternate inside chunks of 2 and 4 blocks and across them."""
    d = bytearray(util.datagen(n_bytes, 0.5, 0.0, 41))
    rnd = random.Random(20261018)
    for lo, hi in ((BLOCK, 2 * BLOCK), (4 * BLOCK, 6 * BLOCK), (8 * BLOCK, 9 * BLOCK), (2 * BLOCK + 1000, 2 * BLOCK + 30000), (7 * BLOCK - 500, 7 * BLOCK + 500)):
        hi = min(hi, n_bytes)
        if lo < hi:
            d[lo:hi] = rnd.randbytes(hi - lo)
    return bytes(d)


# ---------------------------------------------------------------- 1. the frame cases ------------------------------------------------

def test_frame_cases_match_the_twin_and_the_reference():
    data = dict(util.corpus())
    for name, case, level, bsid, checksum, csize in util.FRAME_CASES:
        plain = data[case]
        p = util.frame_prefs(level, bsid, checksum, len(plain) if csize else 0, 1)
        s0 = cstats()
        e, frame = both(plain, p, what=name)
        d = grown(s0)
        assert e == 0, (name, e)
        assert frame == expected_frame(plain, level, bsid, checksum, csize), (name, "differs from the reference's frame")
        info = fi.index(frame)
        nb = info[4]
        assert d[0] + d[1] == nb and d[1] == sum(1 for w in info[3] if w >> 31), (name, d, nb)
        assert d[2] == (1 if nb else 0) and d[3] == (len(plain) if checksum else 0), (name, d)
        he, hint, hused, hgot = fi.host_one_call(frame, len(plain) + 16)
        assert (he, hint, hused, hgot) == (0, 0, len(frame), plain), name
        print(name, len(plain), len(frame), d)


# ---------------------------------------------------------------- 2. frames of several chunks ------------------------------------------------

SIZES = (9 * BLOCK + 777, 6 * BLOCK, 6 * BLOCK + 1)


def default_chunk_blocks(bs):
    mb = int(os.environ.get("LIZARDGPU_CHUNK_MB", "0") or 0)
    mb = mb if 1 <= mb <= 65536 else 256
    return max(1, (mb << 20) // bs)


@pytest.mark.parametrize("level", [10, 15, 21, 30])
def test_multi_chunk_frames(level):
    for n in SIZES:
        plain = mixed(9 * BLOCK + 777)[:n]
        nb = -(-n // BLOCK)
        for checksum in (0, 1):
            want = expected_frame(plain, level, 1, checksum, 1)
            raw = sum(1 for w in fi.index(want)[3] if w >> 31)
            assert 0 < raw < nb, "the data no longer mixes raw and compressed records"
            p = util.frame_prefs(level, 1, checksum, n, 1)
            for chunk in (1, 2, 4, None):
                set_chunk(chunk)
                per = default_chunk_blocks(BLOCK) if chunk is None else chunk
                s0 = cstats()
                e, frame = both(plain, p, what=(level, n, checksum, chunk))
                d = grown(s0)
                assert e == 0 and frame == want, (level, n, checksum, chunk, e)
                assert d == [nb - raw, raw, -(-nb // per), n if checksum else 0], (level, n, checksum, chunk, d)


# ---------------------------------------------------------------- 3. capacity ------------------------------------------------

def test_capacity_below_the_bound_leaves_dst_untouched():
    plain = mixed(9 * BLOCK + 777)[:3 * BLOCK + 5]
    for checksum, csize in ((0, 0), (1, 1)):
        p = util.frame_prefs(10, 1, checksum, len(plain) if csize else 0, 1)
        b = bound_of(len(plain), p)
        s0 = cstats()
        e, body = both(plain, p, b - 1)
        assert e == E_TOO_SMALL and body == bytes([CANARY]) * (b - 1)
        assert grown(s0) == [0, 0, 0, 0]
        assert both(plain, p, b)[0] == 0


def test_one_byte_last_block_at_the_bound():
    """A 1-byte block is a 10-byte record where the bound counted 5: under a content-size header (which saves nothing of the 15
    bytes the bound counts for the header) and behind raw blocks only, the frame does not fit a buffer of exactly the bound."""
    noise = random.Random(77).randbytes(BLOCK + 1)
    for plain, what in ((b"x", "one byte"), (noise, "a raw block and one byte")):
        p = util.frame_prefs(10, 1, 0, len(plain), 1)
        b = bound_of(len(plain), p)
        set_chunk(1)
        seen = {}
        for cap in (b, b + 1, b + 4, b + 5):
            seen[cap - b] = both(plain, p, cap, what=(what, cap - b))[0]
        assert seen == {0: E_TOO_SMALL, 1: E_TOO_SMALL, 4: E_TOO_SMALL, 5: 0}, (what, seen)     # (the twin's answers, derived above)
        # without the content size the header is 8 bytes shorter than the bound counted: the frame fits
        assert both(plain, util.frame_prefs(10, 1, 0, 0, 1), what=what)[0] == 0
        # with a checksum the bound counts 4 more bytes, the frame 4 more: the same answers
        p = util.frame_prefs(10, 1, 1, len(plain), 1)
        b = bound_of(len(plain), p)
        assert both(plain, p, b, what=what)[0] == E_TOO_SMALL and both(plain, p, b + 5, what=what)[0] == 0
        set_chunk(None)
        assert both(plain, util.frame_prefs(10, 1, 0, len(plain), 1), what=what)[0] == E_TOO_SMALL


# ---------------------------------------------------------------- 4. refusals ------------------------------------------------

def test_refusals_are_the_twins():
    import torch
    plain = mixed(9 * BLOCK + 777)[:2 * BLOCK + 9]
    cap = bound_of(len(plain), util.frame_prefs(10, 1, 1, len(plain), 1)) + 64
    linked = util.frame_prefs(10, 1, 0, 0, 0)
    s0 = cstats()
    assert both(plain, linked, cap, "linked above one block")[0] == E_BLOCK_MODE
    assert both(plain[:BLOCK], linked, cap, "linked, one block: written as independent")[0] == 0
    assert both(plain, util.frame_prefs(18, 1, 0, 0, 1), cap, "level 18")[0] == E_LEVEL
    skippable = util.frame_prefs(10, 1, 0, 0, 1)
    skippable.frameInfo.frameType = 1
    assert both(plain, skippable, cap, "frameType 1")[0] == E_FRAME_TYPE
    # block size id 8: the id shrinks to the input where one of the seven sizes holds it ...
    assert both(plain, util.frame_prefs(10, 8, 0, 0, 1), cap, "block size id 8, small input")[0] == 0
    assert grown(s0)[2] == 2, "a refused call launched a chunk"
    # ... and is refused above 256 MiB, before anything is read or written
    L = lib()
    n = (256 << 20) + 1
    p = util.frame_prefs(10, 8, 0, 0, 1)
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = dd.padded(bytes(4096), CANARY)
    dst[:] = CANARY
    r = L.LizardGPU_compressFrame_device(dst.data_ptr() + G, 4096, src.data_ptr(), n, C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert fi.err_of(r) == E_BLOCK_SIZE and bool((dst == CANARY).all())
    host = C.create_string_buffer(4096)
    assert fi.err_of(L.LizardGPU_compressFrame(host, 4096, host, n, C.byref(p))) == E_BLOCK_SIZE     # (refused before src is read)
    # null pointers
    q = util.frame_prefs(10, 1, 0, 0, 1)
    assert fi.err_of(L.LizardGPU_compressFrame_device(None, 1 << 20, src.data_ptr(), 1000, C.byref(q), None)) == E_GENERIC
    assert fi.err_of(L.LizardGPU_compressFrame_device(dst.data_ptr(), 1 << 20, None, 1000, C.byref(q), None)) == E_GENERIC


# ---------------------------------------------------------------- 5. round trip ------------------------------------------------

def test_round_trip_on_the_device_and_through_the_host_decoder():
    import numpy as np
    import torch
    from lizard_amd import api
    plain = mixed(9 * BLOCK + 777)
    src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    for level, checksum, csize, chunk in ((10, True, True, 2), (30, False, False, 4), (21, True, False, None)):
        set_chunk(chunk)
        dst, n = api.compress_frame_device(src, level=level, block_size_id=1, checksum=checksum, content_size=csize)
        frame = dst[:n]
        back = api.decompress_frame_device(frame)
        assert back.numel() == len(plain) and bool((back == src).all()), (level, "the device round trip changed the bytes")
        host = frame.cpu().numpy().tobytes()
        he, hint, hused, hgot = fi.host_one_call(host, len(plain) + 16)
        assert (he, hint, hused) == (0, 0, n) and hgot == plain, level
        info = api.frame_info(host)
        assert info["checksum"] == checksum and info["content_size"] == (len(plain) if csize else 0) and info["independent"]


# ---------------------------------------------------------------- 6. stream ordering ------------------------------------------------

def test_ordered_after_the_producer_and_before_the_consumer_on_a_side_stream():
    import numpy as np
    import torch
    from lizard_amd import api
    plain = mixed(9 * BLOCK + 777)
    want = expected_frame(plain, 10, 1, 0, 1)
    a = np.frombuffer(random.Random(5).randbytes(len(plain)), dtype=np.uint8)
    b = np.frombuffer(plain, dtype=np.uint8) ^ a
    ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    big = torch.ones(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    set_chunk(2)
    with torch.cuda.stream(side):
        for _ in range(8):                                  # work in front of the producer: it has not run when the call is made
            big = big @ big * 1e-4
        src = ta ^ tb                                       # the producer, not synchronised
        dst, n = api.compress_frame_device(src, level=10, block_size_id=1, content_size=True)
        mirror = dst[:n].flip(0)                            # the consumer, on the same stream
    side.synchronize()
    assert n == len(want) and mirror.flip(0).cpu().numpy().tobytes() == want


# ---------------------------------------------------------------- 7. the Python wrapper ------------------------------------------------

def test_python_wrapper_allocates_returns_and_raises():
    import numpy as np
    import torch
    from lizard_amd import _lib, api
    plain = mixed(9 * BLOCK + 777)[:2 * BLOCK + 100]
    src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    dst, n = api.compress_frame_device(src)
    p = util.frame_prefs(10, 0, 0, 0, 1)
    assert dst.is_cuda and dst.dtype == torch.uint8 and dst.numel() == bound_of(len(plain), p)
    assert isinstance(n, int) and dst[:n].cpu().numpy().tobytes() == twin(plain, p, dst.numel())[1]
    mine = torch.empty(dst.numel() + 10, dtype=torch.uint8, device="cuda")
    out, m = api.compress_frame_device(src, level=30, checksum=True, content_size=True, dst=mine)
    assert out is mine and mine[:m].cpu().numpy().tobytes() == twin(plain, util.frame_prefs(30, 0, 1, len(plain), 1), mine.numel())[1]
    with pytest.raises(_lib.LizardAmdError, match="compressionLevel_invalid"):
        api.compress_frame_device(src, level=18)
    with pytest.raises(_lib.LizardAmdError, match="dstMaxSize_tooSmall"):
        api.compress_frame_device(src, dst=mine[:1000])
    empty, z = api.compress_frame_device(torch.empty(0, dtype=torch.uint8, device="cuda"), checksum=True)
    assert empty[:z].cpu().numpy().tobytes() == twin(b"", util.frame_prefs(10, 0, 1, 0, 1), 64)[1]


# ---------------------------------------------------------------- the kernels alone ------------------------------------------------

def test_frame_pack_kernels_against_the_host_model():
    exe = os.path.join(util.ROOT, "tests", "frame_pack_kernels")
    assert os.path.exists(exe), "tests/frame_pack_kernels is built by __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    print(r.stdout.strip())
