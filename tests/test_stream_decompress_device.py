"""LizardGPU_decompressStream_device / LizardGPU_streamIndex_device: a STREAM of frames — back to back in one device buffer — decoded
into one device buffer in batches.  The entry's contract is the loop over LizardGPU_decompressFrame_device; every case here runs that
loop on the same bytes with the same capacity and flags and requires the same return value, consumed bytes, frame count, decoded
count and decoded bytes.  Source and destination lie in torch tensors with 4 KiB canary margins that are checked after every call.
Shapes are the smallest that touch every boundary: block size id 1 (128 KiB) and frames of 0, 1, 131 072, 131 073 and 300 000 bytes,
one of them incompressible so that raw records occur.  The damaged streams are refused by design, by refusals the single-frame
entry already makes; no case here aims at anything else."""
import ctypes as C
import functools
import os
import struct
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
BLOCK = 131072
SKIP_CHECKSUM = dd.SKIP_CHECKSUM
SKIP = dd.SKIP
E_GENERIC, E_TOO_SMALL, E_HEADER_INCOMPLETE, E_FRAME_SIZE, E_CONTENT_CRC = 1, 11, 12, 14, 18
WALK_ENV = "LIZARDGPU_STREAM_WALK_FRAMES"


@pytest.fixture(autouse=True)
def _no_override_left_behind():
    os.environ.pop(WALK_ENV, None)
    yield
    os.environ.pop(WALK_ENV, None)


def lib():
    return dd.lib()


def sstats():
    out = (C.c_ulonglong * 4)()
    assert lib().LizardGPU_streamDecodeDeviceStats(out) == 0
    return list(out)


def grown(s0):
    return [b - a for a, b in zip(s0, sstats())]


@functools.lru_cache(maxsize=None)
def plains():
    """The five inputs: 0, 1, 131 072, 131 073 (noise: raw records) and 300 000 bytes."""
    import random
    d = util.datagen(BLOCK + 300000 + 1, 0.5, 0.0, 61)
    return (b"", d[:1], d[1:1 + BLOCK], random.Random(61).randbytes(BLOCK + 1), d[1 + BLOCK:1 + BLOCK + 300000])


@functools.lru_cache(maxsize=None)
def frames_of(level, checksum, csize, which=(0, 1, 2, 3, 4)):
    """The frames compress_frames_device writes for the inputs `which`, as host bytes."""
    import torch
    from lizard_amd import api
    tensors = [torch.frombuffer(bytearray(plains()[i] or b"\0"), dtype=torch.uint8)[:len(plains()[i])].cuda() for i in which]
    out = api._compress_frames_device(tensors, level, 1, bool(checksum), bool(csize), api.STREAM_FRAME_SLACK)
    return tuple(f.cpu().numpy().tobytes() for f in out)


def placed(stream, cap, odd):
    """(src tensor, dst tensor, offset of the stream / of d_dst in them): 4 KiB margins, `odd`: both start at an odd address."""
    k = 1 if odd else 0
    src, dst = dd.padded(bytes(k) + bytes(stream), 0x5A), dd.padded(bytes(cap + k), CANARY)
    src[G:G + k] = 0x5A
    dst[G:G + cap + k] = CANARY
    assert (src.data_ptr() + G + k) % 2 == k and (dst.data_ptr() + G + k) % 2 == k
    return src, dst, G + k


def checked(src, dst, at, stream, cap):
    """The margins of both tensors and the source are intact; the destination's body."""
    import numpy as np
    hs, hd = src.cpu().numpy(), dst.cpu().numpy()
    assert (hs[:at] == 0x5A).all() and (hs[at + len(stream):] == 0x5A).all() and hs[at:at + len(stream)].tobytes() == bytes(stream), "the source changed"
    assert (hd[:at] == CANARY).all() and (hd[at + cap:] == CANARY).all(), "the decoder wrote outside d_dst[0..dstCapacity)"
    return hd[at:at + cap]


def entry(stream, cap, flags=0, odd=False):
    """(error number or 0, consumed, frames, decoded, bytes d_dst[0..decoded)) of LizardGPU_decompressStream_device."""
    import torch
    L = lib()
    src, dst, at = placed(stream, cap, odd)
    used, frames, decoded = C.c_size_t(12345), C.c_size_t(12345), C.c_size_t(12345)
    stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = L.LizardGPU_decompressStream_device(dst.data_ptr() + at, cap, src.data_ptr() + at, len(stream), C.byref(used), C.byref(frames), C.byref(decoded),
                                            flags, stream_h)
    entry.error_text = L.LizardGPU_lastError()
    body = checked(src, dst, at, stream, cap)
    e = fi.err_of(r)
    assert decoded.value <= cap and (e or r == decoded.value)
    return e, used.value, frames.value, decoded.value, body[:decoded.value].tobytes()


def loop(stream, cap, flags=0, odd=False):
    """The same from the loop over the single-frame device entry that defines the contract."""
    import torch
    L = lib()
    src, dst, at = placed(stream, cap, odd)
    stream_h = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos, out, frames, e = 0, 0, 0, 0
    while pos < len(stream):
        used = C.c_size_t(0)
        r = L.LizardGPU_decompressFrame_device(dst.data_ptr() + at + out, cap - out, src.data_ptr() + at + pos, len(stream) - pos, C.byref(used), flags, stream_h)
        e = fi.err_of(r)
        if e:
            break
        out += r; pos += used.value; frames += 1
    body = checked(src, dst, at, stream, cap)
    return e, pos, frames, out, body[:out].tobytes()


def same_as_loop(stream, cap, flags=0, odd=False, what=None):
    got = entry(stream, cap, flags, odd)
    want = loop(stream, cap, flags, odd)
    assert got[:4] == want[:4], ("stream entry and loop disagree", what, got[:4], want[:4], entry.error_text)
    assert got[4] == want[4], ("decoded bytes differ from the loop's", what)
    return got


# ---------------------------------------------------------------- 1. round trip ------------------------------------------------

@pytest.mark.parametrize("level", [10, 21, 30])
def test_round_trip_of_the_five_tensors_is_one_batch(level):
    import torch
    from lizard_amd import api
    tensors = [torch.frombuffer(bytearray(p or b"\0"), dtype=torch.uint8)[:len(p)].cuda() for p in plains()]
    whole = b"".join(plains())
    for checksum in (False, True):
        stream = api.compress_stream_device(tensors, level=level, block_size_id=1, checksum=checksum)
        assert stream.is_cuda and stream.dtype == torch.uint8 and stream.dim() == 1
        s0 = sstats()
        back, n = api.decompress_stream_device(stream)
        d = grown(s0)
        assert n == 5 and back.cpu().numpy().tobytes() == whole, (level, checksum)
        assert d[1] == 1 and d[2] == 0 and d[0] == 5, ("one batch, nothing handed over", d)      # ([3]: the walk of stream_info_device and the decoder's)
        # the entry itself: consumed bytes are the stream's length; an exact destination, a given size, a larger buffer
        host = stream.cpu().numpy().tobytes()
        s0 = sstats()
        got = same_as_loop(host, len(whole), what=(level, checksum))
        assert got == (0, len(host), 5, len(whole), whole) and grown(s0) == [5, 1, 0, 1]
        back, n = api.decompress_stream_device(stream, size=len(whole), verify_checksum=False)
        assert n == 5 and back.cpu().numpy().tobytes() == whole
        dst = torch.empty(len(whole) + 777, dtype=torch.uint8, device="cuda")
        back, n = api.decompress_stream_device(stream, dst=dst)
        assert n == 5 and back.data_ptr() == dst.data_ptr() and back.cpu().numpy().tobytes() == whole


# ---------------------------------------------------------------- 2. identity with the loop ------------------------------------------------

def test_frames_without_content_size_are_a_batch_each():
    fr = frames_of(10, 1, 0)
    stream, whole = b"".join(fr), b"".join(plains())
    s0 = sstats()
    got = same_as_loop(stream, len(whole) + 100)
    assert got == (0, len(stream), 5, len(whole), whole)
    assert grown(s0) == [5, 4, 0, 1]                           # (the empty frame has no records: its size is known, it shares a batch)


def test_a_mix_of_frames_with_and_without_content_size():
    sized, plain = frames_of(10, 0, 1), frames_of(10, 1, 0)
    order = [sized[4], plain[2], sized[1], sized[3], plain[4], plain[0], sized[2]]
    want = b"".join(plains()[i] for i in (4, 2, 1, 3, 4, 0, 2))
    stream = b"".join(order)
    s0 = sstats()
    for cap in (len(want), len(want) + 5):
        assert same_as_loop(stream, cap) == (0, len(stream), 7, len(want), want)
    assert grown(s0) == [14, 6, 0, 2]                          # [s4 p2] [s1 s3 p4] [p0 s2]


def test_a_skippable_frame_in_the_middle():
    fr = frames_of(21, 1, 1)
    stream = fr[4] + SKIP + fr[3] + struct.pack("<II", 0x184D2A50, 0) + fr[1]
    want = plains()[4] + plains()[3] + plains()[1]
    s0 = sstats()
    assert same_as_loop(stream, len(want)) == (0, len(stream), 5, len(want), want)
    assert grown(s0) == [5, 1, 0, 1]


def test_the_same_source_frame_twice():
    fr = frames_of(30, 1, 1)
    stream = fr[4] + fr[4] + fr[3] + fr[4]
    want = plains()[4] * 2 + plains()[3] + plains()[4]
    assert same_as_loop(stream, len(want)) == (0, len(stream), 4, len(want), want)


def test_seven_frames_with_walk_segments_of_three():
    fr = frames_of(10, 1, 1)
    order = (4, 0, 1, 3, 2, 1, 4)
    stream, want = b"".join(fr[i] for i in order), b"".join(plains()[i] for i in order)
    os.environ[WALK_ENV] = "3"
    s0 = sstats()
    assert same_as_loop(stream, len(want)) == (0, len(stream), 7, len(want), want)
    assert grown(s0) == [7, 1, 0, 3], "one batch across three walk segments"
    os.environ[WALK_ENV] = "1"
    s0 = sstats()
    assert same_as_loop(stream, len(want))[:4] == (0, len(stream), 7, len(want))
    assert grown(s0) == [7, 1, 0, 7]


def test_a_stream_that_starts_at_an_odd_device_address():
    for level, checksum, csize in ((10, 1, 1), (30, 0, 0)):
        fr = frames_of(level, checksum, csize)
        stream, whole = b"".join(fr), b"".join(plains())
        assert same_as_loop(stream, len(whole), odd=True) == (0, len(stream), 5, len(whole), whole)
        assert same_as_loop(stream, len(whole) - 1, odd=True)[0] == E_TOO_SMALL


# ---------------------------------------------------------------- 3. interop ------------------------------------------------

def reference_decode(stream, cap):
    """LizardF_decompress of the compiled reference, frame after frame: the decoded bytes."""
    ref = util.reference()
    ref.LizardF_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]; ref.LizardF_createDecompressionContext.restype = C.c_size_t
    ref.LizardF_freeDecompressionContext.argtypes = [C.c_void_p]
    ref.LizardF_decompress.restype = C.c_size_t
    ref.LizardF_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    dctx = C.c_void_p()
    assert ref.LizardF_createDecompressionContext(C.byref(dctx), 100) == 0
    back, src = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(bytes(stream), len(stream))
    so, do, frames = 0, 0, 0
    while so < len(stream):
        ds, ss = C.c_size_t(cap - do), C.c_size_t(len(stream) - so)
        r = ref.LizardF_decompress(dctx, C.byref(back, do), C.byref(ds), C.byref(src, so), C.byref(ss), None)
        assert r < (1 << 63), "the reference's frame decoder refused the stream"
        assert ss.value or ds.value, "the reference's frame decoder made no progress"
        so += ss.value; do += ds.value
        frames += 1 if r == 0 else 0
    ref.LizardF_freeDecompressionContext(dctx)
    return back.raw[:do], frames


def test_the_reference_decodes_a_stream_written_here():
    import torch
    from lizard_amd import api
    if util.reference() is None:
        util.need_ref("oracle/_ref/liblizard_ref_reset.so")
    tensors = [torch.frombuffer(bytearray(p or b"\0"), dtype=torch.uint8)[:len(p)].cuda() for p in plains()]
    whole = b"".join(plains())
    for level, checksum in ((10, True), (30, False)):
        stream = api.compress_stream_device(tensors, level=level, block_size_id=1, checksum=checksum).cpu().numpy().tobytes()
        back, frames = reference_decode(stream, len(whole))
        assert frames == 5 and back == whole, (level, checksum)


def test_a_stream_of_reference_made_frames_decodes_here():
    """Three frames of the compiled reference, the middle one in linked mode: the device never settles a linked frame of several
    blocks, the single-frame entry finishes it on the host, and [2] counts it."""
    if util.reference() is None:
        util.need_ref("oracle/_ref/liblizard_ref_reset.so")
    a, b, c = plains()[4], plains()[2] + plains()[4][:70000], plains()[3]
    stream = util.reference_frame(a, util.frame_prefs(10, 1, 1, len(a), 1)) + util.reference_frame(b, util.frame_prefs(17, 1, 1, 0, 0)) \
        + util.reference_frame(c, util.frame_prefs(30, 1, 0, 0, 1))
    s0, f0 = sstats(), dd.dstats()
    assert same_as_loop(stream, len(a + b + c)) == (0, len(stream), 3, len(a + b + c), a + b + c)
    d = grown(s0)
    assert d[2] == 1 and d[0] == 2 and d[1] == 2, d
    assert dd.grown(f0)[2] >= 2, "the linked frame was not finished on the host (by the entry and by the loop)"


def test_a_stream_of_the_committed_reference_frames():
    (_, linked, plain, _), (_, independent, plain2, _) = fd.reference_frames()
    stream = independent + linked + frames_of(10, 1, 1)[4]
    want = plain2 + plain + plains()[4]
    s0 = sstats()
    assert same_as_loop(stream, len(want) + 9) == (0, len(stream), 3, len(want), want)
    assert grown(s0)[2] == 1, "the linked frame is the single-frame entry's"


# ---------------------------------------------------------------- 4. damage ------------------------------------------------

@functools.lru_cache(maxsize=None)
def four():
    """(frames, plains) of the damage cases: 131 072 P50, 131 073 noise, 300 000 P50, 1 byte; content size and checksum."""
    fr = frames_of(10, 1, 1)
    order = (2, 3, 4, 1)
    return [fr[i] for i in order], [plains()[i] for i in order]


def refused(stream, cap, flags, ahead, code, what):
    """Identity with the loop; the refusal is frame `ahead`'s; the bytes of the frames in front of it are intact."""
    fr, pl = four()
    got = same_as_loop(stream, cap, flags, what=what)
    front = b"".join(pl[:ahead])
    assert got[0] and (code is None or got[0] == code), (what, got[:4])
    assert got[1:] == (sum(len(f) for f in fr[:ahead]), ahead, len(front), front), (what, got[:4])
    return got


def test_a_wrong_stored_checksum_in_frame_two_of_four():
    fr, pl = four()
    bad = fr[1][:-1] + bytes([fr[1][-1] ^ 0x40])
    stream = fr[0] + bad + fr[2] + fr[3]
    total = sum(len(p) for p in pl)
    refused(stream, total, 0, 1, E_CONTENT_CRC, "wrong checksum")
    assert same_as_loop(stream, total, SKIP_CHECKSUM) == (0, len(stream), 4, total, b"".join(pl)), "verification off: the stored checksum is not looked at"
    from lizard_amd import api, LizardAmdError
    import numpy as np
    import torch
    t = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    with pytest.raises(LizardAmdError, match="frame 1 at offset %d: .*contentChecksum_invalid" % len(fr[0])):
        api.decompress_stream_device(t)
    back, n = api.decompress_stream_device(t, verify_checksum=False)
    assert n == 4 and back.cpu().numpy().tobytes() == b"".join(pl)


def test_a_flipped_byte_inside_a_compressed_block_of_frame_three():
    fr, pl = four()
    rc, _, offs, words, _, _ = fi.index(fr[2])
    assert rc == 0 and not words[0] >> 31, "the first record of frame 3 is a compressed block"
    at = offs[0] + (words[0] & 0x7FFFFFFF) // 2
    bad = fr[2][:at] + bytes([fr[2][at] ^ 0xFF]) + fr[2][at + 1:]
    refused(fr[0] + fr[1] + bad + fr[3], sum(len(p) for p in pl), 0, 2, None, "flipped byte")


@pytest.mark.parametrize("cut", [1, 5])
def test_a_truncated_stream(cut):
    fr, pl = four()
    stream = b"".join(fr)[:-cut]
    refused(stream, sum(len(p) for p in pl), 0, 3, E_GENERIC, ("truncated", cut))


def test_capacity_short_of_the_total():
    fr, pl = four()
    total = sum(len(p) for p in pl)
    refused(b"".join(fr), total - 1, 0, 3, E_TOO_SMALL, "one byte short")
    refused(b"".join(fr), len(pl[0]) + len(pl[1]), 0, 2, E_TOO_SMALL, "room for the first two frames")


def test_a_content_size_one_more_than_the_truth():
    import xxhash
    fr, pl = four()
    f = bytearray(fr[1])
    assert f[4] & 8 and struct.unpack_from("<Q", f, 6)[0] == len(pl[1])
    struct.pack_into("<Q", f, 6, len(pl[1]) + 1)
    f[14] = (xxhash.xxh32(bytes(f[4:14]), seed=0).intdigest() >> 8) & 255
    assert fi.index(bytes(f))[0] == 0
    stream = fr[0] + bytes(f) + fr[2] + fr[3]
    refused(stream, sum(len(p) for p in pl) + 1, 0, 1, E_FRAME_SIZE, "content size + 1")
    refused(stream, sum(len(p) for p in pl), 0, 1, None, "content size + 1, no room to spare")


# ---------------------------------------------------------------- 5. the index ------------------------------------------------

def test_stream_info_equals_frames_info_plus_offsets():
    import numpy as np
    import torch
    from lizard_amd import api, LizardAmdError
    fr = list(frames_of(10, 1, 1)) + [SKIP] + list(frames_of(21, 0, 0))
    stream = b"".join(fr)
    t = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    for env in (None, "4"):
        if env:
            os.environ[WALK_ENV] = env
        got = api.stream_info_device(t)
        singles = api.frames_info_device([torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in fr])
        pos = 0
        assert len(got) == len(singles) == 11
        for g, s, f in zip(got, singles, fr):
            assert g == dict(s, offset=pos), (pos, g, s)
            pos += len(f)
        assert pos == len(stream)
    with pytest.raises(LizardAmdError, match="frame 11 at offset %d" % len(stream)):
        api.stream_info_device(torch.cat([t, t[:9]]))
    assert api.stream_info_device(t[:0]) == []
