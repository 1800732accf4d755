"""api.compress_tensors_device(..., planes="bits") / decompress_tensors_device / tensors_info_device on the GPU: the mixed list of
tests/test_tensor_stream_gpu.py — bf16 [1000, 37], fp32 [3], int64 [0], uint8 [5], an fp16 scalar, int32 [131073], bool [17] — with
element BITS split into planes, one frame each behind an "LZT2" tensor header.  Dtype, shape and bytes come back exactly at levels
10 / 21 / 30, with and without checksum; tensors_info_device says "bits" and the element sizes; the stream is ONE decode batch; the
frame decoders — this library's and the reference's — yield the numpy bit-plane bytes (which pins the layout independently of the
kernel); a stream concatenated from a "bytes" stream and a "bits" stream decodes, with one join launch per filter; damaged headers
raise naming the tensor; planes="bits" with split=False, or another value, raises ValueError; and fp16 / bf16 weights shrink as the
reference library says they do."""
import ctypes as C
import functools
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import bitplanes_inputs as bi
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


def counter(name, k):
    out = (C.c_ulonglong * 4)()
    from lizard_amd import _lib
    assert getattr(_lib.lib(), name)(out) == 0
    return out[k]


def batches():
    return counter("LizardGPU_streamDecodeDeviceStats", 1)


def launches():
    """(byte-plane launches, bit-plane launches) so far."""
    return counter("LizardGPU_planesStats", 3), counter("LizardGPU_bitPlanesStats", 3)


@pytest.mark.parametrize("checksum", (False, True))
@pytest.mark.parametrize("level", (10, 21, 30))
def test_round_trip_of_a_mixed_list(level, checksum):
    import torch
    a = api()
    host = host_tensors()
    l0 = launches()
    stream = a.compress_tensors_device([t.cuda() for t in host], level=level, checksum=checksum, planes="bits")
    assert launches() == (l0[0], l0[1] + 1), "not ONE bit-split launch and no byte-split launch"
    assert stream.dtype == torch.uint8 and stream.is_cuda and stream.dim() == 1
    info = a.tensors_info_device(stream)
    assert [(i["dtype"], i["shape"], i["nbytes"]) for i in info] == [(str(t.dtype).split(".")[-1], tuple(t.shape), t.numel() * t.element_size()) for t in host]
    assert [i["planes"] for i in info] == ["bits"] * len(host)
    assert [i["elem_size"] for i in info] == list(ELEMS)
    assert [i["header_bytes"] for i in info] == [48 + 8 * t.dim() for t in host]
    pos = 0
    data = stream.cpu().numpy().tobytes()
    for i in info:
        assert i["offset"] == pos and data[pos + 8:pos + 12] == b"LZT2" and data[pos + 14:pos + 16] == b"\1\0"
        pos += i["header_bytes"] + i["frame_bytes"]
    assert pos == stream.numel()
    b0, l0 = batches(), launches()
    back = a.decompress_tensors_device(stream)
    assert batches() == b0 + 1, "the stream was not ONE decode batch"
    assert launches() == (l0[0], l0[1] + 1), "not ONE bit-join launch and no byte-join launch"
    assert len(back) == len(host)
    for t, b in zip(host, back):
        assert b.is_cuda and b.dtype == t.dtype and tuple(b.shape) == tuple(t.shape) and b.is_contiguous()
        assert b.data_ptr() % 256 == 0 or not b.numel()
        assert np.array_equal(raw_bytes(b.cpu()), raw_bytes(t)), (t.dtype, tuple(t.shape))
    if checksum:                                                 # and without verifying it
        again = a.decompress_tensors_device(stream, verify_checksum=False)
        assert all(np.array_equal(raw_bytes(b.cpu()), raw_bytes(t)) for t, b in zip(host, again))


def test_the_default_and_planes_bytes_are_the_stream_of_before():
    """planes="bytes" is the default, writes "LZT1" headers through Write2 and reports "bytes"."""
    import torch
    a = api()
    host = host_tensors()
    dev = [t.cuda() for t in host]
    default = a.compress_tensors_device(dev, level=10, checksum=True)
    named = a.compress_tensors_device(dev, level=10, checksum=True, planes="bytes")
    assert torch.equal(default, named)
    info = a.tensors_info_device(default)
    assert [i["planes"] for i in info] == ["bytes"] * len(host) and [i["elem_size"] for i in info] == list(ELEMS)
    data = default.cpu().numpy().tobytes()
    assert all(data[i["offset"] + 8:i["offset"] + 16] == b"LZT1" + bytes([E, len(t.shape), 0, 0]) for i, E, t in zip(info, ELEMS, host))
    want = b"".join(pi.split_model(raw_bytes(t), E).tobytes() for t, E in zip(host, ELEMS))
    plain, _ = a.decompress_stream_device(default)
    assert plain.cpu().numpy().tobytes() == want
    for kw in ({"planes": "bits", "split": False}, {"planes": "bit"}, {"planes": None}, {"planes": 1}):
        with pytest.raises(ValueError):
            a.compress_tensors_device(dev, level=10, **kw)


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
def test_the_container_is_a_liz_stream_of_the_numpy_bit_plane_bytes(level):
    a = api()
    host = host_tensors()
    stream = a.compress_tensors_device([t.cuda() for t in host], level=level, checksum=True, planes="bits")
    want = b"".join(bi.bits_split_model(raw_bytes(t), E).tobytes() for t, E in zip(host, ELEMS))
    plain, frames = a.decompress_stream_device(stream)
    assert frames == 2 * len(host) and plain.cpu().numpy().tobytes() == want
    assert reference_decode(stream.cpu().numpy().tobytes()) == want


def test_a_stream_of_both_kinds_of_tensor_decodes_with_one_join_launch_each():
    import torch
    a = api()
    host = host_tensors()
    dev = [t.cuda() for t in host]
    by = a.compress_tensors_device(dev, level=10, planes="bytes")
    bt = a.compress_tensors_device(dev, level=30, checksum=True, planes="bits")
    unsplit = a.compress_tensors_device(dev[:2], level=10, split=False)
    stream = torch.cat([by, bt, unsplit, bt])
    info = a.tensors_info_device(stream)
    n = len(host)
    assert [i["planes"] for i in info] == ["bytes"] * n + ["bits"] * n + ["bytes"] * 2 + ["bits"] * n
    assert [i["elem_size"] for i in info] == list(ELEMS) * 2 + [1, 1] + list(ELEMS)
    b0, l0 = batches(), launches()
    back = a.decompress_tensors_device(stream)
    assert batches() == b0 + 1, "the stream was not ONE decode batch"
    assert launches() == (l0[0] + 1, l0[1] + 1), "not one byte-join launch and one bit-join launch"
    want = list(host) * 2 + list(host[:2]) + list(host)
    assert len(back) == len(want)
    for t, b in zip(want, back):
        assert b.dtype == t.dtype and tuple(b.shape) == tuple(t.shape) and (b.data_ptr() % 256 == 0 or not b.numel())
        assert np.array_equal(raw_bytes(b.cpu()), raw_bytes(t)), (t.dtype, tuple(t.shape))


def test_damaged_headers_raise_naming_the_tensor():
    import torch
    from lizard_amd import _lib
    a = api()
    host = host_tensors()
    stream = a.compress_tensors_device([t.cuda() for t in host], level=10, planes="bits")
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
        refused(data[:o + hb] + FOREIGN + data[o + hb:], k)                  # ... and one between it and the data frame
        changed = struct.pack("<Q", info[k]["nbytes"] + 2)
        refused(data[:o + 16] + changed + data[o + 24:], k)                  # the header's nbytes changed
        refused(data[:o + 14] + b"\0" + data[o + 15:], k)                    # "LZT2" with the byte-plane filter: no encoding of anything
        refused(data[:o + 14] + b"\2" + data[o + 15:], k)                    # a filter nobody knows
        refused(data[:o + 15] + b"\1" + data[o + 16:], k)                    # a non-zero byte 7
        refused(data[:o + 8] + b"LZT1" + data[o + 12:], k)                   # "LZT1" with a filter byte
        refused(data[:o + 8] + b"LZT3" + data[o + 12:], k, a.tensors_info_device)
    o = info[5]["offset"]
    refused(data[:o + 24] + b"int33".ljust(24, b"\0") + data[o + 48:], 5)    # a dtype torch does not know
    refused(data[:o + 8 + 40] + struct.pack("<Q", 131072) + data[o + 8 + 48:], 5)   # a shape that is not nbytes
    # the intact stream still reads
    assert len(a.decompress_tensors_device(torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda())) == len(host)


def test_fp16_and_bf16_weights_shrink_with_bit_planes_at_level_10():
    """randn(2^19) * 0.02, generated on the CPU with manual_seed(1), level 10, block_size_id 0.  The reference library gives for
    this generator's values (scripts/bitplanes_ratio.py): fp16 0.9375 x raw with bit planes and 1.0000 with byte planes, bf16 0.7645
    with bit planes and 0.8431 with byte planes; the margins to 0.96 / 0.99 / 0.80 cover only another torch generator."""
    import torch
    a = api()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = torch.randn(2 ** 19) * 0.02
    raw = w.numel() * 2
    size = {}
    for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        t = w.to(dt).cuda()
        for planes in ("bits", "bytes"):
            s = a.compress_tensors_device([t], level=10, block_size_id=0, planes=planes)
            size[name, planes] = int(s.numel())
            back, = a.decompress_tensors_device(s)
            assert back.dtype == dt and torch.equal(back.view(torch.int16), t.view(torch.int16))
        print("%s randn * 0.02, level 10: bits %.4f, bytes %.4f of %d raw bytes" % (name, size[name, "bits"] / raw, size[name, "bytes"] / raw, raw))
    assert size["fp16", "bits"] <= 0.96 * raw
    assert size["fp16", "bytes"] >= 0.99 * raw
    assert size["bf16", "bits"] <= 0.80 * raw
    assert size["bf16", "bits"] < size["bf16", "bytes"]
