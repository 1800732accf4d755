"""LizardGPU_compressFrames_device: many buffers that lie in device memory, one Lizard frame each, in one batch.  Every case also runs
the host-memory twin LizardGPU_compressFrame on each buffer with the same preferences and capacity and requires the same result and
the same frame bytes for every frame of the batch; at levels 10 and 30 the frames are also compared with the reference's (or its
restatement over the oracle's blocks).  All sources lie in one torch tensor and all destinations in another, 4 KiB canary margins
around every one of them, checked after every call.  The helpers are those of test_frame_compress_device."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_frame_compress_device as fc

pytestmark = pytest.mark.gpu

G = fc.G
CANARY = fc.CANARY
BLOCK = fc.BLOCK
KIB = 1024
E_GENERIC, E_BLOCK_MODE, E_LEVEL, E_TOO_SMALL = fc.E_GENERIC, fc.E_BLOCK_MODE, fc.E_LEVEL, fc.E_TOO_SMALL
ERR_ARG = 3


@pytest.fixture(autouse=True)
def _no_chunk_override_left_behind():
    yield
    os.environ.pop(fc.CHUNK_ENV, None)


def prefs_of(n, level, bsid, checksum, csize, independent=1):
    """The preferences of the twin's call for a buffer of n bytes: the batch says "write each frame's own size" with any non-zero value."""
    return util.frame_prefs(level, bsid, checksum, n if csize else 0, independent)


def laid_out(sizes, fill, odd):
    """(host array, positions): regions of `sizes` bytes with 4 KiB of `fill` around each; odd: every region starts at an odd address
    of its own residue mod 16."""
    import numpy as np
    pos, at = G, []
    for i, n in enumerate(sizes):
        if odd:
            pos += (2 * i + 1) % 16 + (16 - pos % 16) % 16      # 1, 3, 5, .. bytes behind a 16-byte boundary
        at.append(pos)
        pos += n + G
    return np.full(pos, fill, dtype=np.uint8), at


def batch(bufs, level, bsid, checksum, csize, independent=1, cap_deltas=None, odd=False, null_dst=None):
    """One call on torch's current stream.  Returns (return value, [(error number or 0, frame bytes or the whole region) per frame]);
    every byte outside the destinations' capacities and the sources themselves checked."""
    import numpy as np
    import torch
    L = fc.lib()
    n = len(bufs)
    caps = [fc.bound_of(len(b), prefs_of(len(b), level, bsid, checksum, csize, independent)) + (cap_deltas[i] if cap_deltas else 0) for i, b in enumerate(bufs)]
    hsrc, spos = laid_out([len(b) for b in bufs], 0x5A, odd)
    hdst, dpos = laid_out(caps, CANARY, odd)
    for b, at in zip(bufs, spos):
        hsrc[at:at + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    src, dst = torch.from_numpy(hsrc).cuda(), torch.from_numpy(hdst).cuda()
    dsts = (C.c_void_p * n)(*[None if i == null_dst else dst.data_ptr() + at for i, at in enumerate(dpos)])
    srcs = (C.c_void_p * n)(*[src.data_ptr() + at for at in spos])
    results = (C.c_size_t * n)(*([12345] * n))
    p = util.frame_prefs(level, bsid, checksum, 1 if csize else 0, independent)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.LizardGPU_compressFrames_device(n, dsts, (C.c_size_t * n)(*caps), srcs, (C.c_size_t * n)(*[len(b) for b in bufs]), results, C.byref(p), stream)
    batch.error_text = L.LizardGPU_lastError()              # (the twins' calls that follow clear it)
    assert (src.cpu().numpy() == hsrc).all(), "a source or its margins changed"
    got = dst.cpu().numpy()
    out = []
    for at, cap, r in zip(dpos, caps, results):
        e = fi.err_of(r)
        assert e or r <= cap
        out.append((e, got[at:at + (cap if e else r)].tobytes()))
        hdst[at:at + cap] = got[at:at + cap]
    assert (got == hdst).all(), "the batch wrote outside a destination's capacity"
    return rc, out


def same_as_the_twins(bufs, level, bsid, checksum, csize, independent=1, cap_deltas=None, odd=False, what=None):
    """The batch and, per buffer, the host twin: the same results, the same frames.  Returns the batch's list."""
    rc, out = batch(bufs, level, bsid, checksum, csize, independent, cap_deltas, odd)
    assert rc == 0, (what, rc, batch.error_text)
    for i, (b, (e, frame)) in enumerate(zip(bufs, out)):
        p = prefs_of(len(b), level, bsid, checksum, csize, independent)
        cap = fc.bound_of(len(b), p) + (cap_deltas[i] if cap_deltas else 0)
        te, want = fc.twin(b, p, cap)
        assert e == te, ("batch and host twin disagree", what, i, len(b), e, te, batch.error_text)
        if not e:
            assert frame == want, ("the frames differ", what, i, len(b), len(frame), len(want))
    return out


def buffers():
    """0, 1, 15, 16, 17, 128 KiB - 1, 128 KiB, 128 KiB + 1 bytes of P50, and 3 x 128 KiB + 5 bytes in which raw and compressed records alternate."""
    plain = util.datagen(3 * BLOCK + 64, 0.5, 0.0, 23)
    out, at = [], 0
    for n in (0, 1, 15, 16, 17, BLOCK - 1, BLOCK, BLOCK + 1):
        out.append(plain[at:at + n])
        at += n
    return out + [fc.mixed(9 * BLOCK + 777)[:3 * BLOCK + 5]]


def runs_of_blocks():
    """Frames of 3, 1, 0, 2 and 5 blocks, cut from the data that mixes raw and compressed records."""
    d = fc.mixed(9 * BLOCK + 777)
    return [d[:3 * BLOCK], d[3 * BLOCK:4 * BLOCK], b"", d[4 * BLOCK:6 * BLOCK], d[4 * BLOCK + 777:9 * BLOCK + 777]]


# ---------------------------------------------------------------- 1. identity ------------------------------------------------

@pytest.mark.parametrize("level", [10, 15, 21, 30])
def test_every_frame_of_a_batch_is_the_twins(level):
    bufs = buffers()
    s0 = fc.cstats()
    for checksum in (0, 1):
        for csize in (0, 1):
            out = same_as_the_twins(bufs, level, 1, checksum, csize, what=(level, checksum, csize))
            assert [e for e, _ in out] == [0, E_TOO_SMALL if csize else 0] + [0] * 7, out and [e for e, _ in out]      # (the 1-byte frame at its bound under a content-size header)
            if level in (10, 30):
                for b, (e, frame) in zip(bufs, out):
                    assert e or frame == fc.expected_frame(b, level, 1, checksum, csize), (level, len(b), "differs from the reference's frame")
    d = fc.grown(s0)
    assert d[3] == 0, "source bytes were copied to the host"
    assert d[0] + d[1] == 4 * 12 - 2 and d[1] >= 4, d            # 12 blocks per batch; the 1-byte frames that were refused are in no count


# ---------------------------------------------------------------- 2. chunks ------------------------------------------------

def test_chunk_borders_inside_and_between_frames():
    bufs = runs_of_blocks()
    total = sum(-(-len(b) // BLOCK) for b in bufs)
    first = None
    for chunk in (1, 2, 4, None):
        fc.set_chunk(chunk)
        per = fc.default_chunk_blocks(BLOCK) if chunk is None else chunk
        s0 = fc.cstats()
        out = same_as_the_twins(bufs, 10, 1, 1, 1, what=("chunk", chunk))
        d = fc.grown(s0)
        assert all(e == 0 for e, _ in out)
        assert d[0] + d[1] == total and d[1] >= 2 and d[2] == -(-total // per) and d[3] == 0, (chunk, d)
        first = first or out
        assert out == first, ("the bytes depend on the blocks per chunk", chunk)


# ---------------------------------------------------------------- 3. mixed block sizes ------------------------------------------------

def test_every_frame_gets_the_block_size_of_its_own_input():
    d = util.datagen((1 << 20) + 1, 0.5, 0.0, 31)
    bufs = [d[:100 * KIB], d[:200 * KIB], d[:300 * KIB], d]
    for level in (10, 21):
        out = same_as_the_twins(bufs, level, 4, 1, 1, what=("block size id 4", level))
        assert [e for e, _ in out] == [0, 0, 0, 0]
        assert [fi.index(frame)[1].blockSizeID for _, frame in out] == [1, 2, 3, 4]


# ---------------------------------------------------------------- 4. unaligned ------------------------------------------------

def test_sources_and_destinations_at_odd_addresses():
    for level, checksum in ((10, 1), (30, 0)):
        same_as_the_twins(buffers(), level, 1, checksum, 0, odd=True, what=("odd addresses", level))
    fc.set_chunk(2)
    same_as_the_twins(runs_of_blocks(), 10, 1, 1, 1, odd=True, what="odd addresses, frames of several chunks")


# ---------------------------------------------------------------- 5. capacity and refusals ------------------------------------------------

def test_a_refused_frame_does_not_stop_the_others():
    bufs = runs_of_blocks()
    s0 = fc.cstats()
    # one frame one byte below its bound among good ones: only it is refused, its region untouched
    out = same_as_the_twins(bufs, 10, 1, 1, 0, cap_deltas=[0, 5, 0, -1, 0], what="one below its bound")
    assert [e for e, _ in out] == [0, 0, 0, E_TOO_SMALL, 0]
    assert out[3][1] == bytes([CANARY]) * len(out[3][1]), "a frame refused below its bound was written to"
    assert b"frame 3 refused" in batch.error_text and b"dstMaxSize_tooSmall" in batch.error_text
    assert fc.grown(s0)[0] + fc.grown(s0)[1] == 3 + 1 + 5
    # the 1-byte last block behind a raw block at exactly the bound, under a content-size header, inside a batch
    noise = random.Random(77).randbytes(BLOCK + 1)
    out = same_as_the_twins([bufs[1], noise, b"x", bufs[3]], 10, 1, 0, 1, what="1-byte last block at the bound")
    assert [e for e, _ in out] == [0, E_TOO_SMALL, E_TOO_SMALL, 0]
    out = same_as_the_twins([bufs[1], noise, b"x", bufs[3]], 10, 1, 0, 1, cap_deltas=[0, 5, 5, 0], what="1-byte last block, five bytes more")
    assert [e for e, _ in out] == [0, 0, 0, 0]
    # linked blocks: refused above one block, written as independent at one block, as by the twin
    out = same_as_the_twins([bufs[3], bufs[1]], 10, 1, 0, 0, independent=0, what="linked")
    assert [e for e, _ in out] == [E_BLOCK_MODE, 0]
    # level 18: every frame, nothing launched, nothing written
    s0 = fc.cstats()
    out = same_as_the_twins(bufs, 18, 1, 0, 0, what="level 18")
    assert all(e == E_LEVEL and region == bytes([CANARY]) * len(region) for e, region in out) and fc.grown(s0) == [0, 0, 0, 0]
    # a null destination in one entry
    rc, out = batch(bufs, 10, 1, 1, 1, null_dst=1)
    want = same_as_the_twins(bufs, 10, 1, 1, 1, what="after a null destination")
    assert rc == 0 and out[1][0] == E_GENERIC and [o for i, o in enumerate(out) if i != 1] == [o for i, o in enumerate(want) if i != 1]
    # no frames, null arrays
    L = fc.lib()
    assert L.LizardGPU_compressFrames_device(0, None, None, None, None, None, None, None) == 0
    assert L.LizardGPU_compressFrames_device(2, None, None, None, None, None, None, None) == -ERR_ARG


# ---------------------------------------------------------------- 6. round trip and stream order ------------------------------------------------

def test_round_trip_behind_a_producer_that_is_not_waited_for():
    import numpy as np
    import torch
    from lizard_amd import api
    bufs = [b for b in buffers() + runs_of_blocks()]
    rnd = random.Random(5)
    masks = [rnd.randbytes(len(b)) for b in bufs]
    ta = [torch.from_numpy(np.frombuffer(m, dtype=np.uint8).copy()).cuda() for m in masks]
    tb = [torch.from_numpy((np.frombuffer(b, dtype=np.uint8) ^ np.frombuffer(m, dtype=np.uint8)).copy()).cuda() for b, m in zip(bufs, masks)]
    big = torch.ones(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    fc.set_chunk(4)
    with torch.cuda.stream(side):
        for _ in range(8):                                  # work in front of the producers: they have not run when the call is made
            big = big @ big * 1e-4
        srcs = [a ^ b for a, b in zip(ta, tb)]              # the producers, not synchronised
        frames = api.compress_frames_device(srcs, level=10, block_size_id=1, checksum=True, content_size=False)
        backs = [api.decompress_frame_device(f) for f in frames]      # the consumers, on the same stream
    side.synchronize()
    for b, f, back in zip(bufs, frames, backs):
        assert back.cpu().numpy().tobytes() == b, (len(b), "the device round trip changed the bytes")
        host = f.cpu().numpy().tobytes()
        he, hint, hused, hgot = fi.host_one_call(host, len(b) + 16)
        assert (he, hint, hused) == (0, 0, len(host)) and hgot == b, len(b)


# ---------------------------------------------------------------- 7. the Python wrapper ------------------------------------------------

def test_python_wrapper_lays_out_returns_and_raises():
    import numpy as np
    import torch
    from lizard_amd import _lib, api
    bufs = runs_of_blocks() + [b"x"]
    srcs = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() for b in bufs]
    frames = api.compress_frames_device(srcs, level=30, checksum=True)
    assert isinstance(frames, list) and len(frames) == len(bufs)
    at = frames[0].data_ptr()
    assert at % 256 == 0
    for b, f in zip(bufs, frames):
        p = util.frame_prefs(30, 0, 1, 0, 1)
        cap = fc.bound_of(len(b), p)
        assert f.is_cuda and f.dtype == torch.uint8 and f.data_ptr() == at, "regions of bound size at 256-byte-aligned offsets"
        assert f.cpu().numpy().tobytes() == fc.twin(b, p, cap)[1]
        at += (cap + 255) & ~255
    assert frames[0]._base is frames[-1]._base, "one output tensor holds every frame"
    assert api.compress_frames_device([]) == []
    with pytest.raises(_lib.LizardAmdError, match="frame 0.*compressionLevel_invalid"):
        api.compress_frames_device(srcs, level=18)
    with pytest.raises(_lib.LizardAmdError, match="frame 5.*dstMaxSize_tooSmall"):
        api.compress_frames_device(srcs, content_size=True)      # the 1-byte buffer at its bound under a content-size header


# ---------------------------------------------------------------- the kernels alone ------------------------------------------------

def test_frames_pack_kernels_against_the_host_model():
    exe = os.path.join(util.ROOT, "tests", "frames_pack_kernels")
    assert os.path.exists(exe), "tests/frames_pack_kernels is built by __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    print(r.stdout.strip())
