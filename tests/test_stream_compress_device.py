"""LizardGPU_compressStream_device on the GPU, through api.compress_stream_device_into and the two entries that now go through it: many
device buffers, one frame each, back to back in ONE device buffer behind opaque prefixes.  The yardstick is the path this entry
replaces, unchanged code: api._compress_stream_device_cat (LizardGPU_compressFrames_device into bound-sized regions and one torch.cat)
and, for the pieces, api._compress_frames_device.  The batch is the one of test_stream_compress_fake_device: frames of 3, 1, 0, 0, 2
and 5 blocks of 128 KiB, one byte, one block and a byte behind noise (the 10-byte record), and an empty frame at the end; compressible
blocks and blocks of noise, which are stored raw."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_tensor_stream_gpu as ts

pytestmark = pytest.mark.gpu

BLOCK = 131072
G = 4096
CANARY = 0xC3
CHUNK_ENV = "LIZARDGPU_FRAME_CHUNK_BLOCKS"
E_GENERIC, E_BLOCK_MODE, E_LEVEL, E_TOO_SMALL = 1, 3, 5, 11
FRAMES = [(0, 3 * BLOCK), (3 * BLOCK, BLOCK), (0, 0), (0, 0), (4 * BLOCK, 2 * BLOCK), (6 * BLOCK, 5 * BLOCK), (777, 1), (9 * BLOCK - 1, BLOCK + 1), (0, 0)]
TOTAL_BLOCKS = 14


def api():
    from lizard_amd import api as a
    return a


def lib():
    from lizard_amd import _lib
    return _lib.lib()


def err(code):
    return (1 << 64) - code


@pytest.fixture(autouse=True)
def _no_chunk_override_left_behind():
    yield
    os.environ.pop(CHUNK_ENV, None)


@functools.lru_cache(maxsize=None)
def data():
    """P50 with noise across block borders; the block in front of 10 * BLOCK is noise."""
    d = bytearray(util.datagen(12 * BLOCK, 0.5, 0.0, 77))
    rnd = random.Random(20261020)
    for lo, hi in ((2 * BLOCK - 5000, 3 * BLOCK + 4000), (9 * BLOCK, 10 * BLOCK)):
        d[lo:hi] = rnd.randbytes(hi - lo)
    return bytes(d)


def plain():
    return [data()[o:o + n] for o, n in FRAMES]


def tensors(odd=False):
    """The frames' sources as views of ONE uint8 CUDA tensor; odd: every view starts at an odd address of its own residue mod 16."""
    import torch
    pos, at = 0, []
    for i, (_, n) in enumerate(FRAMES):
        pos = (pos + 255) & ~255
        if odd:
            pos += (2 * i + 1) % 16
        at.append(pos)
        pos += n
    host = np.full(pos + 16, 0x5A, dtype=np.uint8)
    for p, b in zip(at, plain()):
        host[p:p + len(b)] = np.frombuffer(b, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    out = [dev[p:p + n] for p, (_, n) in zip(at, FRAMES)]
    assert not odd or all(t.data_ptr() % 2 == 1 for t in out if t.numel())
    return out


def counters(name):
    out = (C.c_ulonglong * 4)()
    assert getattr(lib(), name)(out) == 0
    return list(out)


@functools.lru_cache(maxsize=None)
def old_stream(level, checksum):
    """The parent's way, once per (level, checksum): the stream's bytes and every frame's."""
    a = api()
    os.environ.pop(CHUNK_ENV, None)
    stream = a._compress_stream_device_cat(tensors(), level=level, block_size_id=1, checksum=bool(checksum)).cpu().numpy().tobytes()
    frames = [f.cpu().numpy().tobytes() for f in a._compress_frames_device(tensors(), level, 1, bool(checksum), True, a.STREAM_FRAME_SLACK)]
    assert b"".join(frames) == stream
    return stream, frames


def test_the_entry_exists_and_the_old_path_is_kept():
    L = lib()
    for name in ("LizardGPU_compressStreamBound", "LizardGPU_compressStream_device", "LizardGPU_streamCompressDeviceStats"):
        assert hasattr(L, name), name
    assert callable(api()._compress_stream_device_cat) and callable(api().compress_stream_device_into)


@pytest.mark.parametrize("level", [10, 15, 21, 30])
def test_the_stream_equals_the_old_path(level):
    a = api()
    for checksum in (0, 1):
        want, frames = old_stream(level, checksum)
        s0, f0 = counters("LizardGPU_streamCompressDeviceStats"), counters("LizardGPU_frameCompressDeviceStats")
        got, offsets = a.compress_stream_device_into(tensors(), level=level, block_size_id=1, checksum=bool(checksum))
        d = [y - x for x, y in zip(s0, counters("LizardGPU_streamCompressDeviceStats"))]
        assert counters("LizardGPU_frameCompressDeviceStats") == f0, "LizardGPU_frameCompressDeviceStats moved"
        assert got.cpu().numpy().tobytes() == want, (level, checksum, got.numel(), len(want))
        assert offsets == [sum(len(f) for f in frames[:i]) for i in range(len(frames) + 1)]
        assert d[0] == len(FRAMES) and d[1] >= 2 and d[2] >= 1 and d[3] == 1, d
        assert a.compress_stream_device(tensors(), level=level, block_size_id=1, checksum=bool(checksum)).cpu().numpy().tobytes() == want


@pytest.mark.parametrize("chunk", [1, 3])
def test_chunk_borders_inside_between_and_on_empty_frames(chunk):
    a = api()
    for level, checksum in ((10, 1), (30, 0)):
        want, _ = old_stream(level, checksum)
        os.environ[CHUNK_ENV] = str(chunk)
        s0 = counters("LizardGPU_streamCompressDeviceStats")
        got, _ = a.compress_stream_device_into(tensors(), level=level, block_size_id=1, checksum=bool(checksum))
        assert counters("LizardGPU_streamCompressDeviceStats")[2] - s0[2] == -(-TOTAL_BLOCKS // chunk)
        assert got.cpu().numpy().tobytes() == want, (level, checksum, chunk)


@pytest.mark.parametrize("size", [0, 1, 56])
def test_prefixes_of_0_1_and_56_bytes(size):
    a = api()
    _, frames = old_stream(10, 1)
    prefixes = [bytes((0xA0 + 7 * i + k) & 255 for k in range(size)) for i in range(len(FRAMES))]
    got, offsets = a.compress_stream_device_into(tensors(), prefixes=prefixes, level=10, block_size_id=1, checksum=True)
    assert got.cpu().numpy().tobytes() == b"".join(p + f for p, f in zip(prefixes, frames))
    assert offsets == [sum(size + len(f) for f in frames[:i]) for i in range(len(frames) + 1)]
    # and prefixes of unequal sizes, a long one among them
    prefixes = [bytes([i]) * n for i, n in enumerate((56, 0, 5000, 1, 0, 72, 3, 56, 9))]
    got, offsets = a.compress_stream_device_into(tensors(), prefixes=prefixes, level=10, block_size_id=1, checksum=True)
    assert got.cpu().numpy().tobytes() == b"".join(p + f for p, f in zip(prefixes, frames))


def test_sources_at_odd_addresses():
    a = api()
    for level, checksum in ((10, 1), (21, 0)):
        want, _ = old_stream(level, checksum)
        os.environ[CHUNK_ENV] = "3"
        got, _ = a.compress_stream_device_into(tensors(odd=True), level=level, block_size_id=1, checksum=bool(checksum))
        os.environ.pop(CHUNK_ENV)
        assert got.cpu().numpy().tobytes() == want, (level, checksum)


def test_the_stream_decodes_in_one_batch():
    a = api()
    for checksum in (False, True):
        stream, _ = a.compress_stream_device_into(tensors(), level=10, block_size_id=1, checksum=checksum)
        b0 = counters("LizardGPU_streamDecodeDeviceStats")[1]
        back, frames = a.decompress_stream_device(stream)
        assert counters("LizardGPU_streamDecodeDeviceStats")[1] == b0 + 1, "the stream was not ONE decode batch"
        assert frames == len(FRAMES) and back.cpu().numpy().tobytes() == b"".join(plain())


def test_the_reference_decoder_reads_the_stream():
    stream, _ = api().compress_stream_device_into(tensors(), level=30, block_size_id=1, checksum=True)
    assert ts.reference_decode(stream.cpu().numpy().tobytes()) == b"".join(plain())
    # and with prefixes that are skippable frames, as tensor headers are
    prefixes = [ts.FOREIGN] * len(FRAMES)
    stream, _ = api().compress_stream_device_into(tensors(), prefixes=prefixes, level=10, block_size_id=1)
    assert ts.reference_decode(stream.cpu().numpy().tobytes()) == b"".join(plain())


def guarded(cap):
    import torch
    whole = torch.full((cap + 2 * G,), CANARY, dtype=torch.uint8, device="cuda")
    return whole, whole[G:G + cap]


def test_capacity_exact_one_below_and_the_bound():
    from lizard_amd import _lib
    a = api()
    L = lib()
    for checksum in (0, 1):
        want, _ = old_stream(10, checksum)
        n = len(FRAMES)
        sizes = (C.c_size_t * n)(*[s for _, s in FRAMES])
        p = util.frame_prefs(10, 1, checksum, 1, 1)
        bound = L.LizardGPU_compressStreamBound(n, sizes, None, C.byref(p))
        assert bound == sum(L.LizardGPU_compressFrameBound(s, C.byref(p)) + 8 for _, s in FRAMES)
        for cap in (len(want), bound):
            whole, dst = guarded(cap)
            got, _ = a.compress_stream_device_into(tensors(), dst=dst, level=10, block_size_id=1, checksum=bool(checksum))
            assert got.data_ptr() == dst.data_ptr() and got.cpu().numpy().tobytes() == want
            w = whole.cpu().numpy()
            assert (w[:G] == CANARY).all() and (w[G + cap:] == CANARY).all(), "written outside d_dst"
        whole, dst = guarded(len(want) - 1)
        with pytest.raises(_lib.LizardAmdError, match="dstMaxSize_tooSmall"):
            a.compress_stream_device_into(tensors(), dst=dst, level=10, block_size_id=1, checksum=bool(checksum))
        w = whole.cpu().numpy()
        assert (w[:G] == CANARY).all() and (w[G + len(want) - 1:] == CANARY).all(), "written outside d_dst"
    # the allocation of a call without dst is the bound, and the result a view of it
    out = a.compress_stream_device(tensors(), level=10, block_size_id=1, checksum=True)
    assert out.untyped_storage().nbytes() == bound and out.numel() == len(want)


def raw_call(srcs, sizes, p, cap=None):
    """LizardGPU_compressStream_device itself on torch's current stream, into a guarded buffer: (return value, failedFrame, buffer as bytes)."""
    import torch
    L = lib()
    n = len(sizes)
    csizes = (C.c_size_t * n)(*sizes)
    cap = L.LizardGPU_compressStreamBound(n, csizes, None, C.byref(p)) if cap is None else cap
    whole, dst = guarded(cap)
    failed = C.c_size_t(777)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = L.LizardGPU_compressStream_device(dst.data_ptr(), cap, n, (C.c_void_p * n)(*srcs), csizes, None, None, C.byref(p), None, C.byref(failed), stream)
    return r, failed.value, whole.cpu().numpy()


def test_a_frame_refused_up_front_stops_the_call():
    from lizard_amd import _lib
    L = lib()
    t = tensors()
    ptrs, sizes = [x.data_ptr() for x in t], [s for _, s in FRAMES]
    s0 = counters("LizardGPU_streamCompressDeviceStats")
    # level 23 has no kernel: frame 0 decides
    r, failed, w = raw_call(ptrs, sizes, util.frame_prefs(23, 1, 0, 1, 1))
    assert (r, failed) == (err(E_LEVEL), 0) and (w == CANARY).all()
    assert b"frame 0 refused" in L.LizardGPU_lastError()
    # linked mode: frames of one block or less are written independent, the first of two blocks is refused; the one of five behind it changes nothing
    pick = [1, 2, 4, 5]
    r, failed, w = raw_call([ptrs[i] for i in pick], [sizes[i] for i in pick], util.frame_prefs(10, 1, 1, 1, 0))
    assert (r, failed) == (err(E_BLOCK_MODE), 2) and (w == CANARY).all()
    # a null source with a size (an empty frame's null source in front of it is none); a second one behind it changes nothing
    nulls = [None if i in (2, 4, 7) else q for i, q in enumerate(ptrs)]
    r, failed, w = raw_call(nulls, sizes, util.frame_prefs(10, 1, 0, 1, 1))
    assert (r, failed) == (err(E_GENERIC), 4) and (w == CANARY).all()
    assert counters("LizardGPU_streamCompressDeviceStats") == s0, "a refused call launched something"
    # no frames; null arrays
    assert L.LizardGPU_compressStream_device(None, 0, 0, None, None, None, None, None, None, None, None) == 0
    assert L.LizardGPU_compressStream_device(t[0].data_ptr(), 100, 2, None, None, None, None, None, None, None, None) == err(E_GENERIC)
    assert L.LizardGPU_lastError() != b""
    # the wrapper raises naming the frame
    with pytest.raises(_lib.LizardAmdError, match="compressionLevel_invalid.*frame 0"):
        api().compress_stream_device(t, level=23)


def test_round_trip_behind_a_producer_that_is_not_waited_for():
    import torch
    a = api()
    bufs = plain()
    rnd = random.Random(5)
    masks = [rnd.randbytes(len(b)) for b in bufs]
    ta = [torch.from_numpy(np.frombuffer(m, dtype=np.uint8).copy()).cuda() for m in masks]
    tb = [torch.from_numpy((np.frombuffer(b, dtype=np.uint8) ^ np.frombuffer(m, dtype=np.uint8)).copy()).cuda() for b, m in zip(bufs, masks)]
    big = torch.ones(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    os.environ[CHUNK_ENV] = "4"
    with torch.cuda.stream(side):
        for _ in range(8):                                  # work in front of the producers: they have not run when the call is made
            big = big @ big * 1e-4
        srcs = [x ^ y for x, y in zip(ta, tb)]              # the producers, not synchronised
        stream, _ = a.compress_stream_device_into(srcs, level=10, block_size_id=1, checksum=True)
        back, frames = a.decompress_stream_device(stream)   # the consumer, on the same stream
    side.synchronize()
    assert frames == len(bufs) and back.cpu().numpy().tobytes() == b"".join(bufs)
    assert stream.cpu().numpy().tobytes() == old_stream(10, 1)[0]


@functools.lru_cache(maxsize=None)
def host_tensors():
    import torch
    g = torch.Generator().manual_seed(9)
    return (
        (torch.randn(300, 331, generator=g) * 0.02).to(torch.bfloat16),      # more than one block
        torch.randn(1000, 37, generator=g),
        torch.randint(0, 256, (5,), generator=g).to(torch.uint8),
        torch.empty(0, dtype=torch.float32),
        torch.randint(0, 7, (BLOCK + 1,), generator=g).to(torch.uint8),      # a block and a byte
        (torch.randn(3, generator=g)).to(torch.bfloat16),
    )


@pytest.mark.parametrize("planes", ["bytes", "bits"])
def test_tensor_streams_equal_the_old_composition(planes):
    import torch
    a = api()
    L = lib()
    host = host_tensors()
    dev = [t.cuda() for t in host]
    bits = planes == "bits"
    for level, checksum in ((10, True), (30, False)):
        got = a.compress_tensors_device(dev, level=level, checksum=checksum, planes=planes)
        # what compress_tensors_device did before: the split, the batch of frames into regions of their own, the headers, one torch.cat
        raw = [a._as_bytes(t) for t in dev]
        elems = [a._plane_elem_size(t) for t in dev]
        if bits:
            raw = a.split_bit_planes_device(raw, elems)
        else:
            wide = [i for i, e in enumerate(elems) if e > 1]
            for i, p in zip(wide, a.split_planes_device([raw[i] for i in wide], [elems[i] for i in wide])):
                raw[i] = p
        frames = a._compress_frames_device(raw, level, 0, checksum, True, a.STREAM_FRAME_SLACK)
        parts = []
        for t, e, f in zip(host, elems, frames):
            d = a._TensorDesc()
            d.elemSize, d.ndim, d.nbytes, d.dtype = e, t.dim(), t.numel() * t.element_size(), str(t.dtype).split(".")[-1].encode()
            d.filter = a.FILTER_BIT_PLANES if bits else a.FILTER_BYTE_PLANES
            for k, s in enumerate(t.shape):
                d.shape[k] = int(s)
            buf = C.create_string_buffer(a.TENSOR_HEADER_MAX)
            n = L.LizardGPU_tensorHeaderWrite2(buf, a.TENSOR_HEADER_MAX, C.byref(d))
            assert n
            parts += [buf.raw[:n], f.cpu().numpy().tobytes()]
        assert got.cpu().numpy().tobytes() == b"".join(parts), (planes, level, checksum)
        assert got.dtype == torch.uint8 and got.is_cuda and got.dim() == 1
        back = a.decompress_tensors_device(got)
        assert len(back) == len(host)
        for t, b in zip(host, back):
            assert b.dtype == t.dtype and tuple(b.shape) == tuple(t.shape)
            assert np.array_equal(ts.raw_bytes(b.cpu()), ts.raw_bytes(t)), (t.dtype, tuple(t.shape))


def test_stream_pack_kernels_against_the_host_model():
    exe = os.path.join(util.ROOT, "tests", "stream_pack_kernels")
    assert os.path.exists(exe), "tests/stream_pack_kernels is built by __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    print(r.stdout.strip())
