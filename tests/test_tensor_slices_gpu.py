"""GPU: api.decompress_tensor_slices_device and the C entries under it (include/lizard_amd.h Part 3d: LizardGPU_decompressFrameRanges_device,
LizardGPU_joinPlanesRange_device; lz_unslice_kernel, lz_planes_range_kernel).  Seven tensors — bf16 (1000, 200): 4 blocks of 128 KiB with
the plane boundary inside block 1; fp32 (300, 250); fp16 (4099, 7) and int64 (4099,): n % 8 != 0; uint8 (300000,); bf16 (7, 8): one
block; bf16 (0, 5): empty — in one seekable stream, written with byte planes and bit planes at levels 10 and 30, once unsplit and once
with a base for every tensor.  Per tensor: all rows, none, the first row, the last row, a range that crosses a block edge in as many
planes as the tensor allows (in EVERY plane for the first tensor with byte planes) and a range inside a single block of every plane.
Every result is torch.equal, on uint8 views, to decompress_tensors_device(select=[k])[0][start:stop], with its dtype and shape, and
LizardGPU_sliceDeviceStats()[0] grows by exactly the blocks that LizardGPU_planesRangeBytes and the block size predict.  A damaged
picked block raises naming the tensor, the same damage in a block that is not picked does not; the C entries write nothing outside
their destination at exact capacity and nothing at all at capacity - 1; a stream without a table raises."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util

pytestmark = pytest.mark.gpu

B = 131072
G, CANARY = 4096, 0xC3
ERR_ARG = 3


def api():
    from lizard_amd import api as a
    return a


def lib():
    from lizard_amd import _lib
    return _lib.lib()


def error():
    from lizard_amd import _lib
    return _lib.LizardAmdError


@functools.lru_cache(maxsize=None)
def tensors():
    import torch
    g = torch.Generator().manual_seed(7)
    out = [(torch.randn(1000, 200, generator=g) * 0.02).to(torch.bfloat16),
           torch.randn(300, 250, generator=g) * 0.02,
           (torch.randn(4099, 7, generator=g) * 0.02).to(torch.float16),
           torch.randint(-1000, 1000, (4099,), generator=g, dtype=torch.int64),
           torch.randint(0, 7, (300000,), generator=g, dtype=torch.int32).to(torch.uint8),
           (torch.randn(7, 8, generator=g) * 0.02).to(torch.bfloat16),
           torch.empty(0, 5, dtype=torch.bfloat16)]
    return [t.cuda() for t in out]


@functools.lru_cache(maxsize=None)
def bases():
    """An earlier version of every tensor: the tensor a step back (w + step)."""
    import torch
    out = []
    for t in tensors():
        step = (torch.ones_like(t, dtype=torch.float32) * 0.001).to(t.dtype) if t.is_floating_point() else torch.ones_like(t)
        out.append((t + step).contiguous())
    return out


@functools.lru_cache(maxsize=None)
def stream(planes, level, split=True, based=False):
    """(the seekable stream, the whole tensors out of it: the reference, computed once per configuration)"""
    a = api()
    kw = dict(level=level, split=split, seekable=True)
    if split:
        kw["planes"] = planes
    if based:
        kw.update(base=bases(), base_tag=41)
    s = a.compress_tensors_device(tensors(), **kw)
    n = len(tensors())
    whole = [a.decompress_tensors_device(s, select=[k], base=bases() if based else None, base_tag=41 if based else None)[0] for k in range(n)]
    for w, t in zip(whole, tensors()):
        assert w.dtype == t.dtype and w.shape == t.shape and bytes_equal(w, t)
    return s, whole


def bytes_equal(x, y):
    import torch
    return torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))


def ranges_of(info, start, stop):
    """The byte ranges of rows [start, stop) of a tensor of the stream, by the product's arithmetic (tests/test_planes_range.py checks it)."""
    rows = info["shape"][0]
    E = info["elem_size"]
    row = info["nbytes"] // rows if rows else 0
    return api().planes_range_bytes(info["nbytes"] // E, E, info["planes"], start * row // E, stop * row // E)


def blocks(ranges):
    return sum((-(-hi // B) - lo // B) for lo, hi in ranges if hi > lo)


def crossing(ranges):
    return sum(1 for lo, hi in ranges if hi > lo and lo // B != (hi - 1) // B)


def slices_for(info):
    """all rows, none, the first row, the last row, the range that crosses a block edge in the most planes, a range inside one block of every plane"""
    rows = info["shape"][0]
    if not rows:
        return [(0, 0)] * 6
    cands = [(a, b) for a in sorted({0, 1, rows // 4, rows // 3, rows // 2}) for b in sorted({rows // 2 + 1, 2 * rows // 3, 3 * rows // 4, rows - 1, rows}) if a < b]
    across = max(cands, key=lambda c: (crossing(ranges_of(info, *c)), -(c[1] - c[0])))
    inside = next(((r, r + 1) for r in range(rows // 2, rows) if not crossing(ranges_of(info, r, r + 1))), (rows - 1, rows))
    return [(0, rows), (rows // 2, rows // 2), (0, 1), (rows - 1, rows), across, inside]


def slice_stats():
    out = (C.c_ulonglong * 4)()
    assert lib().LizardGPU_sliceDeviceStats(out) == 0
    return list(out)


def check_stream(s, whole, based=False):
    a = api()
    infos = a.tensors_info_device(s, seek=True)
    per_tensor = [slices_for(i) for i in infos]
    kw = dict(base=bases(), base_tag=41) if based else {}
    for kind in range(6):
        want_blocks = sum(blocks(ranges_of(i, *sl[kind])) for i, sl in zip(infos, per_tensor))
        s0 = slice_stats()
        got = a.decompress_tensor_slices_device(s, [(k, *sl[kind]) for k, sl in enumerate(per_tensor)], **kw)
        d = [y - x for x, y in zip(s0, slice_stats())]
        assert d == [want_blocks, len(infos), 0, 1], (kind, d, want_blocks)
        assert len(got) == len(whole)
        for k, (g, w, sl) in enumerate(zip(got, whole, per_tensor)):
            want = w[sl[kind][0]:sl[kind][1]]
            assert g.dtype == want.dtype and g.shape == want.shape and bytes_equal(g, want), (k, kind, sl[kind])
            assert g.data_ptr() % 256 == 0
    return infos, per_tensor


@pytest.mark.parametrize("level", (10, 30))
@pytest.mark.parametrize("planes", ("bytes", "bits"))
def test_every_slice_is_the_slice_of_the_whole_tensor(planes, level):
    s, whole = stream(planes, level)
    infos, per_tensor = check_stream(s, whole)
    if planes == "bytes":
        # the first tensor: 4 blocks, the plane boundary inside block 1, and a range that crosses a block edge in EVERY plane
        assert infos[0]["nbytes"] == 400000 and 200000 // B == 1
        assert crossing(ranges_of(infos[0], *per_tensor[0][4])) == 2
    assert all(crossing(ranges_of(i, *sl[5])) == 0 for i, sl in zip(infos, per_tensor))
    # a subset of the tensors, in one call
    a = api()
    got = a.decompress_tensor_slices_device(s, [(1, 10, 20), (4, 5, 131080)])
    assert bytes_equal(got[0], whole[1][10:20]) and bytes_equal(got[1], whole[4][5:131080])


def test_a_stream_written_unsplit():
    s, whole = stream("bytes", 10, split=False)
    infos, _ = check_stream(s, whole)
    assert all(i["elem_size"] == 1 and i["planes"] == "bytes" for i in infos)


@pytest.mark.parametrize("planes", ("bytes", "bits"))
def test_a_base_for_every_tensor(planes):
    s, whole = stream(planes, 10, based=True)
    infos, _ = check_stream(s, whole, based=True)
    assert all(i["xor_base"] for i in infos)
    a = api()
    with pytest.raises(error(), match="tensor 2.*base"):
        a.decompress_tensor_slices_device(s, [(2, 0, 1)])
    with pytest.raises(error(), match="tensor 2.*tag"):
        a.decompress_tensor_slices_device(s, [(2, 0, 1)], base=bases(), base_tag=40)
    with pytest.raises(ValueError):
        a.decompress_tensor_slices_device(s, [(2, 0, 1)], base=bases()[:3])


def test_arguments_that_are_refused():
    import torch
    a = api()
    s, _ = stream("bytes", 10)
    for bad in ([(0, 5, 4)], [(0, 0, 1001)], [(0, -1, 4)], [(1, 0, 1), (1, 1, 2)], [(2, 0, 1), (1, 0, 1)]):
        with pytest.raises(ValueError):
            a.decompress_tensor_slices_device(s, bad)
    assert a.decompress_tensor_slices_device(s, []) == []
    scalar = a.compress_tensors_device([torch.ones((), device="cuda"), torch.ones(3, device="cuda")], seekable=True)
    with pytest.raises(ValueError, match="tensor 0"):
        a.decompress_tensor_slices_device(scalar, [(0, 0, 0)])
    assert bytes_equal(a.decompress_tensor_slices_device(scalar, [(1, 1, 3)])[0], torch.ones(2, device="cuda"))
    # a stream without a table
    plain = a.compress_tensors_device(tensors())
    with pytest.raises(error(), match="no usable seek table"):
        a.decompress_tensor_slices_device(plain, [(0, 0, 1)])


def records_of(frame):
    """[(payload offset in the frame, size, stored raw)] of a frame with content size (a 15-byte header)."""
    out, at = [], 15
    while True:
        word = int.from_bytes(frame[at:at + 4], "little")
        if not word:
            return out
        out.append((at + 4, word & 0x7FFFFFFF, bool(word >> 31)))
        at += 4 + (word & 0x7FFFFFFF)


def test_damage_in_a_picked_block_raises_and_outside_it_does_not():
    """The first byte of a compressed block is its level, which the block decoder checks: flipped, that block fails.  In a picked block
    the slice entry refuses the frame and the tensor is named; in a block of the same frame that is not picked it is not seen (the
    stated limit)."""
    import torch
    a = api()
    s, whole = stream("bytes", 10)
    info = a.tensors_info_device(s, seek=True)[0]
    at = info["offset"] + info["header_bytes"]
    frame = s[at:at + info["frame_bytes"]].cpu().numpy().tobytes()
    recs = records_of(frame)
    assert len(recs) == 4
    rows = (700, 701)                                             # plane 0 in block 1, plane 1 in block 2
    picked = sorted({b for lo, hi in ranges_of(info, *rows) for b in range(lo // B, (hi - 1) // B + 1)})
    assert picked == [1, 2]
    hit = next(b for b in picked if not recs[b][2])
    miss = next(b for b in (0, 3) if not recs[b][2])
    for b, raises in ((hit, True), (miss, False)):
        bad = s.clone()
        bad[at + recs[b][0]] ^= 0xFF
        if raises:
            with pytest.raises(error(), match="tensor 0.*decompressionFailed"):
                a.decompress_tensor_slices_device(bad, [(0, *rows)])
        else:
            got = a.decompress_tensor_slices_device(bad, [(0, *rows)])[0]
            assert bytes_equal(got, whole[0][rows[0]:rows[1]])
            with pytest.raises(error()):                          # the whole-tensor entry decodes that block and refuses
                a.decompress_tensors_device(bad, select=[0])
        # the other tensors of the call are answered either way
    got = a.decompress_tensor_slices_device(s, [(0, *rows), (1, 3, 9)])
    assert bytes_equal(got[1], whole[1][3:9])


class Range(C.Structure):
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_uint64)]


def test_the_c_entries_with_canaries_at_exact_capacity_and_one_byte_less():
    import torch
    a, L = api(), lib()
    s, whole = stream("bits", 10)
    infos = a.tensors_info_device(s, seek=True)
    picks = [(0, 300, 700), (2, 5, 4099), (3, 4090, 4099)]
    split = []                                                    # the full split bytes of the picked frames: the single-frame entry's
    frames, flat = (a._SliceFrame * len(picks))(), []
    for i, (k, start, stop) in enumerate(picks):
        at = infos[k]["offset"] + infos[k]["header_bytes"]
        split.append(a.decompress_frame_device(s[at:at + infos[k]["frame_bytes"]]).cpu().numpy())
        r = ranges_of(infos[k], start, stop)
        frames[i].d_src, frames[i].srcSize, frames[i].firstRange, frames[i].nRanges = s.data_ptr() + at, infos[k]["frame_bytes"], len(flat), len(r)
        flat += r
    arr = (Range * len(flat))(*[Range(lo, hi) for lo, hi in flat])
    need = sum(L.LizardGPU_frameRangesBound(C.byref(arr, frames[i].firstRange * 16), frames[i].nRanges, B) for i in range(len(picks)))
    assert need == blocks(flat) * B
    stream_ptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for cap in (need, need - 1):
        dst = torch.full((cap + 2 * G,), CANARY, dtype=torch.uint8, device="cuda")
        range_at, results = (C.c_uint64 * (len(flat) + 1))(), (C.c_size_t * len(picks))()
        rc = L.LizardGPU_decompressFrameRanges_device(dst.data_ptr() + G, cap, len(picks), frames, arr, range_at, results, stream_ptr)
        got = dst.cpu().numpy()
        assert (got[:G] == CANARY).all() and (got[G + cap:] == CANARY).all()
        if cap < need:
            assert rc == -ERR_ARG and b"dstMaxSize_tooSmall" in L.LizardGPU_lastError() and (got == CANARY).all()
            assert all(L.LizardGPU_frameIsError(r) for r in results)
            continue
        assert rc == 0 and list(results) == [0] * len(picks) and range_at[len(flat)] == need
        for i in range(len(picks)):
            for q in range(frames[i].nRanges):
                r = frames[i].firstRange + q
                lo, hi = flat[r]
                assert (got[G + range_at[r] + lo % B:G + range_at[r] + lo % B + hi - lo] == split[i][lo:hi]).all(), (i, q)
        # the join out of those pieces, into a destination of exactly the range's bytes
        k, start, stop = picks[1]
        info, i = infos[k], 1
        E, row = info["elem_size"], info["nbytes"] // info["shape"][0]
        nbytes = (stop - start) * row
        out = torch.full((nbytes + 2 * G,), CANARY, dtype=torch.uint8, device="cuda")
        item = (a._PlanesRange * 1)()
        item[0].d_dst, item[0].d_base, item[0].nElems, item[0].first, item[0].last = out.data_ptr() + G, None, info["nbytes"] // E, start * row // E, stop * row // E
        item[0].elemSize, item[0].filter, item[0].firstPiece = E, 1, 0
        pieces = (C.c_void_p * frames[i].nRanges)(*[dst.data_ptr() + G + range_at[frames[i].firstRange + q] + flat[frames[i].firstRange + q][0] % B
                                                    for q in range(frames[i].nRanges)])
        assert L.LizardGPU_joinPlanesRange_device(1, item, pieces, stream_ptr) == 0, L.LizardGPU_lastError()
        joined = out.cpu().numpy()
        assert (joined[:G] == CANARY).all() and (joined[G + nbytes:] == CANARY).all()
        assert joined[G:G + nbytes].tobytes() == whole[k][start:stop].contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()
        item[0].elemSize = 3
        assert L.LizardGPU_joinPlanesRange_device(1, item, pieces, stream_ptr) == -ERR_ARG
