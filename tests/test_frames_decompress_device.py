"""LizardGPU_decompressFrames_device / LizardGPU_framesInfo_device: many frames that lie in device memory, each decoded into its own
device buffer, in one batch.  Every case also runs the single-frame entry LizardGPU_decompressFrame_device on each frame with the same
capacity and flags and requires the same result, consumed count and bytes for every frame of the batch.  All sources lie in one torch
tensor and all destinations in another, 4 KiB canary margins around every one of them, checked after every call.  The helpers are those
of test_frame_decompress_device, test_frames_compress_device and test_frame_index.  The damaged frames come from the generators of
those files: the decoder refuses them by design, and no case here aims at anything else."""
import ctypes as C
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
import test_frames_compress_device as fcs

pytestmark = pytest.mark.gpu

G = dd.G
CANARY = dd.CANARY
BLOCK = fcs.BLOCK
SKIP_CHECKSUM = dd.SKIP_CHECKSUM
E_GENERIC, E_TOO_SMALL, E_CONTENT_CRC, E_HEADER_CRC = 1, 11, 18, 17
ERR_ARG = 3
SKIP = dd.SKIP


def ustats():
    out = (C.c_ulonglong * 4)()
    assert dd.lib().LizardGPU_framesDecodeDeviceStats(out) == 0
    return list(out)


def grown(s0):
    return [b - a for a, b in zip(s0, ustats())]


def batch(frames, caps, flags=0, odd=False, null_dst=None, consumed=True):
    """One call on torch's current stream.  Returns (return value, [(error number or 0, consumed, bytes) per frame]); every byte
    outside the destinations' capacities and the sources themselves checked."""
    import numpy as np
    import torch
    L = dd.lib()
    n = len(frames)
    hsrc, spos = fcs.laid_out([len(f) for f in frames], 0x5A, odd)
    hdst, dpos = fcs.laid_out(caps, CANARY, odd)
    for f, at in zip(frames, spos):
        hsrc[at:at + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
    src, dst = torch.from_numpy(hsrc).cuda(), torch.from_numpy(hdst).cuda()
    dsts = (C.c_void_p * n)(*[None if i == null_dst else dst.data_ptr() + at for i, at in enumerate(dpos)])
    srcs = (C.c_void_p * n)(*[src.data_ptr() + at for at in spos])
    results, used = (C.c_size_t * n)(*([12345] * n)), (C.c_size_t * n)(*([12345] * n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.LizardGPU_decompressFrames_device(n, dsts, (C.c_size_t * n)(*caps), srcs, (C.c_size_t * n)(*[len(f) for f in frames]), results,
                                             used if consumed else None, flags, stream)
    batch.error_text = L.LizardGPU_lastError()
    assert (src.cpu().numpy() == hsrc).all(), "a source or its margins changed"
    got = dst.cpu().numpy()
    out = []
    for at, cap, r, u in zip(dpos, caps, results, used):
        e = fi.err_of(r)
        assert e or r <= cap
        if e and consumed:
            assert u == 0
        out.append((e, 0 if e or not consumed else u, b"" if e else got[at:at + r].tobytes()))
        hdst[at:at + cap] = got[at:at + cap]
    assert (got == hdst).all(), "the batch wrote outside a destination's capacity"
    return rc, out


def same_as_single(frames, caps, flags=0, odd=False, what=None):
    """The batch and, per frame, the single-frame entry: the same results, consumed counts and bytes.  Returns the batch's list."""
    rc, out = batch(frames, caps, flags, odd)
    assert rc == 0, (what, rc, batch.error_text)
    text = batch.error_text
    for i, (f, cap, got) in enumerate(zip(frames, caps, out)):
        want = dd.device_only(f, cap, flags)
        assert got == want, ("batch and single-frame entry disagree", what, i, len(f), cap, got[:2], want[:2], text)
    return out


def frames_of(bufs, level, bsid, checksum, csize):
    """The frames LizardGPU_compressFrames_device writes for bufs, as host bytes."""
    rc, out = fcs.batch(bufs, level, bsid, checksum, csize)
    assert rc == 0
    return [(b, frame) for b, (e, frame) in zip(bufs, out) if not e]


# ---------------------------------------------------------------- 1. identity ------------------------------------------------

@pytest.mark.parametrize("level", [10, 21, 30])
def test_every_frame_of_a_batch_is_the_single_entrys(level):
    bufs = fcs.buffers() + fcs.runs_of_blocks()
    for checksum in (0, 1):
        for csize in (0, 1):
            pairs = frames_of(bufs, level, 1, checksum, csize)
            assert len(pairs) >= len(bufs) - 1
            frames, plains = [f for _, f in pairs], [b for b, _ in pairs]
            s0 = ustats()
            out = same_as_single(frames, [len(b) + 64 for b in plains], what=(level, checksum, csize))
            d = grown(s0)
            assert [o for o in out] == [(0, len(f), b) for b, f in pairs], (level, checksum, csize)
            assert d[2] == 0 and d[1] == len(frames) and d[3] == 1, ("a frame of this library was delegated", d)
            assert d[0] == sum(fi.index(f)[4] for f in frames), d
            # exactly-sized buffers: the same answers; a last block of ONE byte is compressed to more bytes than its slot has room for, which
            # lz_unframe_record refuses, so those frames (and no others) are handed to the single-frame entry, which decodes them in a staging slot
            s0 = ustats()
            rc, exact = batch(frames, [len(b) for b in plains])
            assert rc == 0 and exact == out, (level, checksum, csize)
            assert grown(s0)[2] == sum(1 for b in plains if len(b) % BLOCK == 1), grown(s0)


# ---------------------------------------------------------------- 2. table borders ------------------------------------------------

def test_borders_of_the_tables():
    """17 checksummed tiny frames (the hash kernel holds 16 per wave), a frame of 65 full blocks between two one-block frames (the walk
    stores 64 records at a time, the settle wave strides by 64), 257 one-byte frames (the finish kernel has 256 lanes per workgroup)."""
    d = util.datagen(65 * BLOCK, 0.5, 0.0, 41)
    tiny = [d[i * 100:i * 100 + 3 + 5 * i] for i in range(17)]
    part1 = frames_of(tiny, 10, 1, 1, 0)
    part2 = frames_of([d[:BLOCK], d, d[BLOCK:2 * BLOCK]], 10, 1, 1, 1)
    part3 = frames_of([d[i:i + 1] for i in range(257)], 10, 1, 0, 0)
    pairs = part1 + part2 + part3
    assert len(pairs) == 17 + 3 + 257 and fi.index(part2[1][1])[4] == 65
    s0 = ustats()
    caps = [len(b) + 64 for b, _ in pairs]                  # (room to spare: a 1-byte block's record is longer than a 1-byte slot)
    rc, out = batch([f for _, f in pairs], caps)
    assert rc == 0 and out == [(0, len(f), b) for b, f in pairs]
    assert grown(s0) == [17 + 67 + 257, len(pairs), 0, 1]
    # a wrong checksum in the 17th tiny frame and in the last frame of the second part: they alone are refused
    frames = [f for _, f in pairs]
    for i in (16, 19):
        frames[i] = frames[i][:-1] + bytes([frames[i][-1] ^ 1])
    rc, out2 = batch(frames, caps)
    assert rc == 0 and [i for i, o in enumerate(out2) if o[0]] == [16, 19] and out2[16][0] == out2[19][0] == E_CONTENT_CRC
    assert [o for i, o in enumerate(out2) if i not in (16, 19)] == [o for i, o in enumerate(out) if i not in (16, 19)]
    assert b"frame 16 refused" in batch.error_text and b"contentChecksum_invalid" in batch.error_text


# ---------------------------------------------------------------- 3. mixed block sizes ------------------------------------------------

def test_frames_of_every_block_size_in_one_batch():
    d = util.datagen((1 << 20) + 1, 0.5, 0.0, 31)
    bufs = [d[:100 * 1024], d[:200 * 1024], d[:300 * 1024], d, d[:2 * 262144 + 9]]
    pairs = frames_of(bufs[:4], 10, 4, 1, 1) + frames_of(bufs[4:], 21, 2, 1, 0)
    frames = [f for _, f in pairs]
    assert [fi.index(f)[1].blockSizeID for f in frames] == [1, 2, 3, 4, 2]
    s0 = ustats()
    out = same_as_single(frames, [len(b) + 64 for b in bufs], what="block size ids 1 to 4")
    assert out == [(0, len(f), b) for b, f in pairs] and grown(s0)[1:3] == [5, 0]


# ---------------------------------------------------------------- 4. unaligned ------------------------------------------------

def test_sources_and_destinations_at_odd_addresses():
    for level, checksum in ((10, 1), (30, 0)):
        pairs = frames_of(fcs.buffers() + fcs.runs_of_blocks(), level, 1, checksum, 0)
        out = same_as_single([f for _, f in pairs], [len(b) + 3 for b, _ in pairs], odd=True, what=("odd addresses", level))
        assert out == [(0, len(f), b) for b, f in pairs]


# ---------------------------------------------------------------- 5. refusals among good frames ------------------------------------------------

def test_a_refused_frame_does_not_stop_the_others():
    bufs = fcs.runs_of_blocks()
    pairs = frames_of(bufs, 10, 1, 1, 1)
    good = [f for _, f in pairs]
    caps = [len(b) + 16 for b in bufs]
    want = same_as_single(good, caps, what="good frames")
    assert want == [(0, len(f), b) for b, f in pairs]
    f0, f3 = good[0], good[3]
    rc, info, offs, words, n, fb = fi.index(f0)
    flushed_data, pieces = dd.flushed_case()
    flushed = fd.flushed_frame(flushed_data, pieces)
    golden = fd.reference_frames()
    corrupt = bytearray(f0)
    first_compressed = next(i for i in range(n) if not words[i] >> 31)
    corrupt[offs[first_compressed]:offs[first_compressed] + 24] = bytes(24)
    no_size = frames_of([bufs[3]], 10, 1, 1, 0)[0][1]
    cases = [                                    # (what, frame, capacity, flags, expected error or None = whatever the single entry says)
        ("capacity one short", f3, len(bufs[3]) - 1, 0, E_TOO_SMALL),
        ("a truncated chain", f0[:len(f0) // 2], caps[0], 0, E_GENERIC),
        ("a bad header checksum", f0[:6] + bytes([f0[6] ^ 0x20]) + f0[7:], caps[0], 0, E_HEADER_CRC),
        ("a corrupt block", bytes(corrupt), caps[0], 0, None),
        ("a wrong content checksum", no_size[:-1] + bytes([no_size[-1] ^ 1]), caps[3], 0, E_CONTENT_CRC),
        ("a wrong content checksum, not verified", no_size[:-1] + bytes([no_size[-1] ^ 1]), caps[3], SKIP_CHECKSUM, 0),
        ("a skippable frame", SKIP + b"tail", 50, 0, 0),
        ("a flushed frame", flushed, len(flushed_data), 0, 0),
        ("the reference's linked frame", golden[0][1], len(golden[0][2]), 0, 0),
        ("the reference's independent frame", golden[1][1], len(golden[1][2]), 0, 0),
    ]
    for what, frame, cap, flags, expect in cases:
        frames = [good[1], frame, good[4], good[2]]
        s0 = ustats()
        out = same_as_single(frames, [caps[1], cap, caps[4], caps[2]], flags, what=what)
        d = grown(s0)
        assert [out[0], out[2], out[3]] == [want[1], want[4], want[2]], (what, "a neighbour changed")
        if expect is not None:
            assert out[1][0] == expect, (what, out[1][:2])
        if out[1][0]:
            assert b"frame 1 refused" in batch.error_text, (what, batch.error_text)
        else:
            assert batch.error_text == b"", (what, batch.error_text)
        if what in ("capacity one short", "a corrupt block", "a wrong content checksum", "a flushed frame", "the reference's linked frame"):
            assert d[2] == 1 and d[1] == 3, (what, d)            # accepted by the walk, handed to the single-frame entry
        if what in ("a truncated chain", "a skippable frame", "a wrong content checksum, not verified", "the reference's independent frame"):
            assert d[2] == 0, (what, d)
    # without the consumed array
    rc, out = batch(good, caps, consumed=False)
    assert rc == 0 and [(e, b) for e, _, b in out] == [(0, b) for b in bufs]
    # a null destination in one entry
    rc, out = batch(good, caps, null_dst=1)
    assert rc == 0 and out[1][0] == E_GENERIC and [o for i, o in enumerate(out) if i != 1] == [o for i, o in enumerate(want) if i != 1]
    assert b"frame 1 refused" in batch.error_text
    # no frames, null arrays
    L = dd.lib()
    assert L.LizardGPU_decompressFrames_device(0, None, None, None, None, None, None, 0, None) == 0
    assert L.LizardGPU_decompressFrames_device(2, None, None, None, None, None, None, 0, None) == -ERR_ARG
    assert L.LizardGPU_framesInfo_device(0, None, None, None, None, None, None, None) == 0
    assert L.LizardGPU_framesInfo_device(2, None, None, None, None, None, None, None) == -ERR_ARG


# ---------------------------------------------------------------- 6. frames info ------------------------------------------------

def test_frames_info_device_matches_the_host_walk():
    import numpy as np
    import torch
    L = dd.lib()
    rnd = random.Random(dd.SEED)
    bases = fd.intact_frames()
    frames = [f for _, f in bases] + [SKIP, SKIP + b"x", SKIP[:-1], b"", b"\x06\x22\x4d"]
    frames += [fd.damage(rnd, bases[i % len(bases)][1])[1] for i in range(120)]
    n = len(frames)
    hsrc, spos = fcs.laid_out([len(f) for f in frames], 0x5A, True)
    for f, at in zip(frames, spos):
        hsrc[at:at + len(f)] = np.frombuffer(bytes(f), dtype=np.uint8)
    src = torch.from_numpy(hsrc).cuda()
    srcs = (C.c_void_p * n)(*[src.data_ptr() + at for at in spos])
    sizes = (C.c_size_t * n)(*[len(f) for f in frames])
    infos, nrec, fbytes, codes = (util.FrameInfo * n)(), (C.c_size_t * n)(*([7] * n)), (C.c_size_t * n)(*([7] * n)), (C.c_int * n)(*([7] * n))
    for i in range(n):
        infos[i].contentSize = 0xABCD
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.LizardGPU_framesInfo_device(n, srcs, sizes, infos, nrec, fbytes, codes, stream) == 0
    fields = lambda i: (i.blockSizeID, i.blockMode, i.contentChecksumFlag, i.frameType, i.contentSize)
    refused = 0
    for i, f in enumerate(frames):
        want_info = util.FrameInfo()
        want_info.contentSize = 0xABCD
        wn, wfb = C.c_size_t(0), C.c_size_t(0)
        rc = fi.lib().LizardGPU_frameIndex(bytes(f), len(f), C.byref(want_info), None, None, 0, C.byref(wn), C.byref(wfb))
        assert (codes[i], fields(infos[i]), nrec[i], fbytes[i]) == (rc, fields(want_info), wn.value, wfb.value), (i, len(f))
        refused += rc != 0
    assert refused > 20 and n - refused > 10, (refused, n)
    assert L.LizardGPU_framesInfo_device(n, srcs, sizes, None, None, None, None, stream) == 0


# ---------------------------------------------------------------- 7. round trip and stream order ------------------------------------------------

def test_round_trip_behind_a_producer_that_is_not_waited_for():
    import numpy as np
    import torch
    from lizard_amd import api
    bufs = [b for b in fcs.buffers() + fcs.runs_of_blocks()]
    rnd = random.Random(5)
    masks = [rnd.randbytes(len(b)) for b in bufs]
    ta = [torch.from_numpy(np.frombuffer(m, dtype=np.uint8).copy()).cuda() for m in masks]
    tb = [torch.from_numpy((np.frombuffer(b, dtype=np.uint8) ^ np.frombuffer(m, dtype=np.uint8)).copy()).cuda() for b, m in zip(bufs, masks)]
    big = torch.ones(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(8):                                  # work in front of the producers: they have not run when the call is made
            big = big @ big * 1e-4
        srcs = [a ^ b for a, b in zip(ta, tb)]              # the producers, not synchronised
        frames = api.compress_frames_device(srcs, level=10, block_size_id=1, checksum=True, content_size=False)
        backs = api.decompress_frames_device(frames)        # the consumer, on the same stream
        sized = api.decompress_frames_device(frames, sizes=[len(b) for b in bufs])
        doubled = [t * 2 for t in backs]                    # work enqueued behind the call sees its results
    side.synchronize()
    for b, back, s, d2 in zip(bufs, backs, sized, doubled):
        assert back.cpu().numpy().tobytes() == b and s.cpu().numpy().tobytes() == b, (len(b), "the device round trip changed the bytes")
        assert d2.cpu().numpy().tobytes() == (np.frombuffer(b, dtype=np.uint8) * 2).tobytes()


# ---------------------------------------------------------------- 8. the Python wrapper ------------------------------------------------

def test_python_wrapper_lays_out_returns_and_raises():
    import numpy as np
    import torch
    from lizard_amd import _lib, api
    bufs = fcs.runs_of_blocks() + [b"x"]
    srcs = [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() for b in bufs]
    for csize in (False, True):
        frames = api.compress_frames_device(srcs[:5] if csize else srcs, level=30, checksum=True, content_size=csize)
        infos = api.frames_info_device(frames)
        for f, info in zip(frames, infos):
            host = api.frame_info(f.cpu().numpy().tobytes())
            assert info == {k: v for k, v in host.items() if k != "bound"}
        outs = api.decompress_frames_device(frames)
        assert isinstance(outs, list) and len(outs) == len(frames)
        at = outs[0].data_ptr()
        assert at % 256 == 0
        for b, o, info in zip(bufs, outs, infos):
            region = len(b) if csize else info["n_records"] * _lib.lib().LizardGPU_frameBlockSize(info["block_size_id"])
            assert o.is_cuda and o.dtype == torch.uint8 and (o.numel() == 0 or o.data_ptr() == at), "regions at 256-byte-aligned offsets"
            assert o.cpu().numpy().tobytes() == b
            at += (region + 255) & ~255
        assert outs[0]._base is outs[-1]._base, "one output tensor holds every frame"
    assert api.decompress_frames_device([]) == [] and api.frames_info_device([]) == []
    frames = api.compress_frames_device(srcs, level=10, checksum=True)
    wrong = frames[3].clone()
    wrong[-1] ^= 1
    with pytest.raises(_lib.LizardAmdError, match="frame 3.*contentChecksum_invalid"):
        api.decompress_frames_device(frames[:3] + [wrong] + frames[4:])
    outs = api.decompress_frames_device(frames[:3] + [wrong] + frames[4:], verify_checksum=False)
    assert [o.cpu().numpy().tobytes() for o in outs] == bufs
    with pytest.raises(_lib.LizardAmdError, match="frame 1.*dstMaxSize_tooSmall"):
        api.decompress_frames_device(frames, sizes=[len(b) - (i == 1) for i, b in enumerate(bufs)])
    with pytest.raises(_lib.LizardAmdError, match="frame 2.*behind the frame"):
        api.decompress_frames_device(frames[:2] + [torch.cat([frames[2], frames[2][:5]])] + frames[3:])
    with pytest.raises(_lib.LizardAmdError, match="frame 0"):
        api.frames_info_device([frames[0][:9]])


# ---------------------------------------------------------------- the kernels alone ------------------------------------------------

def test_unframes_kernels_against_the_host_model():
    exe = os.path.join(util.ROOT, "tests", "unframes_kernels")
    assert os.path.exists(exe), "tests/unframes_kernels is built by __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    print(r.stdout.strip())
