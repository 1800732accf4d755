"""api.compress_tensors_device / decompress_tensors_device / tensors_info_device on the GPU: tensors of mixed dtype and shape — element
bytes split into planes, one frame each behind a tensor header — as one .liz stream in device memory, and back.  The list holds
every path: bf16 [1000, 37] (two planes with a ragged end), fp32 [3] (less than a 16-element group), int64 [0] (no bytes), uint8 [5]
(element size 1: never split), an fp16 scalar (no dims), int32 [131073] (four planes, more than one block and more than one tile),
bool [17].  Dtype, shape and bytes come back exactly at levels 10 / 21 / 30, with and without checksum, split on and off; the stream
is ONE decode batch; the reference's frame decoder reads it and yields the numpy-split bytes (which pins the layout independently of
the kernel); damaged streams raise naming the tensor; and bf16 weights shrink with the split and do not without it."""
import ctypes as C
import functools
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import planes_inputs as pi

pytestmark = pytest.mark.gpu

FOREIGN = struct.pack("<II", 0x184D2A57, 9) + b"skippable"


def api():
    from lizard_amd import api as a
    return a


@functools.lru_cache(maxsize=None)
def host_tensors():
    import torch
    g = torch.Generator().manual_seed(3)
    return (
        (torch.randn(1000, 37, generator=g) * 0.02).to(torch.bfloat16),
        torch.randn(3, generator=g),
        torch.empty(0, dtype=torch.int64),
        torch.randint(0, 256, (5,), generator=g).to(torch.uint8),
        torch.tensor(0.333, dtype=torch.float16),
        torch.randint(0, 50000, (131073,), generator=g, dtype=torch.int32),
        torch.randint(0, 2, (17,), generator=g).to(torch.bool),
    )


ELEMS = (2, 4, 8, 1, 2, 4, 1)


def raw_bytes(t):
    import torch
    return t.contiguous().reshape(-1).view(torch.uint8).numpy()


def batches():
    out = (C.c_ulonglong * 4)()
    from lizard_amd import _lib
    assert _lib.lib().LizardGPU_streamDecodeDeviceStats(out) == 0
    return out[1]


@pytest.mark.parametrize("split", (True, False))
@pytest.mark.parametrize("checksum", (False, True))
@pytest.mark.parametrize("level", (10, 21, 30))
def test_round_trip_of_a_mixed_list(level, checksum, split):
    import torch
    a = api()
    host = host_tensors()
    stream = a.compress_tensors_device([t.cuda() for t in host], level=level, checksum=checksum, split=split)
    assert stream.dtype == torch.uint8 and stream.is_cuda and stream.dim() == 1
    info = a.tensors_info_device(stream)
    assert [(i["dtype"], i["shape"], i["nbytes"]) for i in info] == [(str(t.dtype).split(".")[-1], tuple(t.shape), t.numel() * t.element_size()) for t in host]
    assert [i["elem_size"] for i in info] == (list(ELEMS) if split else [1] * len(host))
    assert [i["header_bytes"] for i in info] == [48 + 8 * t.dim() for t in host]
    pos = 0
    for i in info:
        assert i["offset"] == pos
        pos += i["header_bytes"] + i["frame_bytes"]
    assert pos == stream.numel()
    b0 = batches()
    back = a.decompress_tensors_device(stream)
    assert batches() == b0 + 1, "the stream was not ONE decode batch"
    assert len(back) == len(host)
    for t, b in zip(host, back):
        assert b.is_cuda and b.dtype == t.dtype and tuple(b.shape) == tuple(t.shape) and b.is_contiguous()
        assert b.data_ptr() % 256 == 0 or not b.numel()
        assert np.array_equal(raw_bytes(b.cpu()), raw_bytes(t)), (t.dtype, tuple(t.shape))
    if checksum:                                                 # and without verifying it
        again = a.decompress_tensors_device(stream, verify_checksum=False)
        assert all(np.array_equal(raw_bytes(b.cpu()), raw_bytes(t)) for t, b in zip(host, again))


def reference_decode(stream):
    """Every frame of `stream` (bytes) through the reference's LizardF_decompress, one after the other: the decoded bytes joined."""
    path = os.path.join(util.REF_DIR, "liblizard_ref.so")
    if not os.path.exists(path):
        util.need_ref("oracle/_ref/liblizard_ref.so")
    R = C.CDLL(path)
    R.LizardF_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]
    R.LizardF_createDecompressionContext.restype = C.c_size_t
    R.LizardF_decompress.restype = C.c_size_t
    R.LizardF_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    R.LizardF_freeDecompressionContext.argtypes = [C.c_void_p]
    dctx = C.c_void_p()
    assert R.LizardF_createDecompressionContext(C.byref(dctx), 100) == 0
    n, cap = len(stream), 1 << 20
    src, dst = C.create_string_buffer(stream, n), C.create_string_buffer(cap)
    pos, out = 0, []
    while pos < n:
        ds, ss = C.c_size_t(cap), C.c_size_t(n - pos)
        r = R.LizardF_decompress(dctx, dst, C.byref(ds), C.byref(src, pos), C.byref(ss), None)
        assert r < (1 << 63), "the reference's frame decoder refused the stream at %d" % pos
        assert ss.value or ds.value
        pos += ss.value
        out.append(dst.raw[:ds.value])
    assert r == 0, "the stream ends inside a frame"
    R.LizardF_freeDecompressionContext(dctx)
    return b"".join(out)


@pytest.mark.parametrize("level", (10, 30))
def test_the_container_is_a_liz_stream_of_the_numpy_split_bytes(level):
    a = api()
    host = host_tensors()
    stream = a.compress_tensors_device([t.cuda() for t in host], level=level, checksum=True)
    want = b"".join(pi.split_model(raw_bytes(t), E).tobytes() for t, E in zip(host, ELEMS))
    plain, frames = a.decompress_stream_device(stream)
    assert frames == 2 * len(host) and plain.cpu().numpy().tobytes() == want
    assert reference_decode(stream.cpu().numpy().tobytes()) == want
    # unsplit, the same container holds the tensors' own bytes
    stream = a.compress_tensors_device([t.cuda() for t in host], level=level, split=False)
    assert reference_decode(stream.cpu().numpy().tobytes()) == b"".join(raw_bytes(t).tobytes() for t in host)


def test_damaged_streams_raise_naming_the_tensor():
    import torch
    from lizard_amd import _lib
    a = api()
    host = host_tensors()
    stream = a.compress_tensors_device([t.cuda() for t in host], level=10)
    info = a.tensors_info_device(stream)
    data = stream.cpu().numpy().tobytes()

    def refused(damaged, k, fn=a.decompress_tensors_device):
        with pytest.raises(_lib.LizardAmdError) as e:
            fn(torch.frombuffer(bytearray(damaged), dtype=torch.uint8).cuda())
        assert "tensor %d:" % k in str(e.value), str(e.value)

    for k in (0, 2, len(host) - 1):
        o, hb = info[k]["offset"], info[k]["header_bytes"]
        refused(data[:o] + data[o + hb:], k)                                 # the header removed
        refused(data[:o] + data[o + hb:], k, a.tensors_info_device)
        refused(data[:o] + FOREIGN + data[o + hb:], k)                       # a foreign skippable frame in its place
        refused(data[:o] + FOREIGN + data[o:], k)                            # ... and one in front of it
        refused(data[:o + hb] + FOREIGN + data[o + hb:], k)                  # ... and one between it and the data frame
        changed = struct.pack("<Q", info[k]["nbytes"] + 2)
        refused(data[:o + 16] + changed + data[o + 24:], k)                  # the header's nbytes changed
    o = info[5]["offset"]
    refused(data[:o + 24] + b"int33".ljust(24, b"\0") + data[o + 48:], 5)    # a dtype torch does not know
    refused(data[:o + 8 + 40] + struct.pack("<Q", 131072) + data[o + 8 + 48:], 5)   # a shape that is not nbytes
    # the intact stream still reads
    assert len(a.decompress_tensors_device(torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda())) == len(host)


def test_bf16_weights_shrink_with_the_split_and_not_without():
    """bf16 randn(2^19) * 0.02, generated on the CPU with manual_seed(1), level 30, block_size_id 0.  The reference library gives
    0.7456 x raw for the split bytes of this generator's values and 1.0000 unsplit; the margin to 0.80 covers only another torch
    generator."""
    import torch
    a = api()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = (torch.randn(2 ** 19) * 0.02).to(torch.bfloat16)
    raw = w.numel() * 2
    split = a.compress_tensors_device([w.cuda()], level=30, block_size_id=0, split=True)
    plain = a.compress_tensors_device([w.cuda()], level=30, block_size_id=0, split=False)
    print("bf16 randn * 0.02, level 30: split %.4f, unsplit %.4f of %d raw bytes" % (split.numel() / raw, plain.numel() / raw, raw))
    assert split.numel() <= 0.80 * raw
    assert plain.numel() >= 0.99 * raw
    back, = a.decompress_tensors_device(split)
    assert back.dtype == torch.bfloat16 and torch.equal(back.cpu().view(torch.int16), w.view(torch.int16))
