"""GPU: seekable streams (include/lizard_amd.h Part 3b; lizard_amd/csrc/lizard_seek_device.c, lz_stream_seektable_kernel).  Frames of 0, 1,
56, 131 072, 131 073 and 300 000 bytes (block size 128 KiB: 8 blocks), with and without tensor-header-like prefixes.
Writer: the stream is the plain entry's bytes plus LizardGPU_seekTableWrite of the returned offsets, at levels 10 and 30, checksum off
and on, with chunks of 1 and 3 blocks; a capacity that is exactly enough succeeds and one byte less is dstMaxSize_tooSmall with the
canaries intact.  Reader: LizardGPU_decompressSeekableStream_device answers what LizardGPU_decompressStream_device answers — through the
table for an intact stream, through the walk for every damaged or lying table and for a damaged frame — at capacities exact, exact - 1
and 0.  Items: some, all, none, and the three refusals.  Tensor streams: seekable=True read with seek, with select and without either;
seekable=False unchanged.  The reference's CLI decodes a seekable file to the payloads."""
import ctypes as C
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import seek_inputs as si

pytestmark = pytest.mark.gpu

BLOCK = 131072
SIZES = (0, 1, 56, BLOCK, BLOCK + 1, 300000)
G, CANARY = 4096, 0xC3
CHUNK_ENV = "LIZARDGPU_FRAME_CHUNK_BLOCKS"
E_GENERIC, E_BLOCK_MODE, E_TOO_SMALL, E_TYPE, E_SIZE = 1, 3, 11, 13, 14


def api():
    from lizard_amd import api as a
    return a


def lib():
    from lizard_amd import _lib
    return _lib.lib()


def err(code):
    return (1 << 64) - code if lib().LizardGPU_frameIsError(code) else 0


@pytest.fixture(autouse=True)
def _no_chunk_override_left_behind():
    yield
    os.environ.pop(CHUNK_ENV, None)


@functools.lru_cache(maxsize=None)
def plain():
    d = util.datagen(sum(SIZES) + 100, 0.5, 0.0, 909)
    out, pos = [], 3
    for n in SIZES:
        out.append(d[pos:pos + n])
        pos += n
    return out


def tensors():
    import torch
    return [torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if b else torch.empty(0, dtype=torch.uint8, device="cuda") for b in plain()]


def prefixes(kind):
    """None, or per frame a skippable frame the size of a tensor header (56 .. 96 bytes), the third frame without one."""
    if not kind:
        return None
    return [b"" if i == 2 else struct.pack("<II", 0x184D2A57, 48 + 8 * i) + bytes((16 * i + k) & 255 for k in range(48 + 8 * i)) for i in range(len(SIZES))]


def counters(name="LizardGPU_seekDeviceStats"):
    out = (C.c_ulonglong * 4)()
    assert getattr(lib(), name)(out) == 0
    return list(out)


def host(t):
    return t.cpu().numpy().tobytes()


def device(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def table_of(offsets, pre):
    """The table the writer must append, by the product's host codec — which equals the struct model."""
    L = lib()
    n = len(SIZES)
    entries = [(offsets[i], SIZES[i], len(pre[i]) if pre else 0, 0) for i in range(n)]
    arr = (api()._SeekEntry * n)(*[api()._SeekEntry(*e) for e in entries])
    buf = C.create_string_buffer(si.table_bytes(n))
    assert L.LizardGPU_seekTableWrite(buf, len(buf), arr, n) == len(buf)
    assert buf.raw == si.pack_table(entries)
    return buf.raw


@functools.lru_cache(maxsize=None)
def streams(level, checksum, pre):
    """(plain stream, seekable stream, offsets) as bytes, once per configuration."""
    a = api()
    os.environ.pop(CHUNK_ENV, None)
    p, offs = a.compress_stream_device_into(tensors(), prefixes=prefixes(pre), level=level, block_size_id=1, checksum=bool(checksum))
    s, soffs = a.compress_stream_device_into(tensors(), prefixes=prefixes(pre), level=level, block_size_id=1, checksum=bool(checksum), seekable=True)
    assert soffs == offs
    return host(p), host(s), tuple(offs)


# ---- writer ----

@pytest.mark.parametrize("pre", (0, 1))
@pytest.mark.parametrize("checksum", (0, 1))
@pytest.mark.parametrize("level", (10, 30))
def test_the_stream_is_the_plain_entrys_plus_the_table_of_its_offsets(level, checksum, pre):
    a = api()
    p, s, offs = streams(level, checksum, pre)
    assert offs[0] == 0 and offs[-1] == len(p), "frameOffsets[n] is where the table starts"
    assert s[:len(p)] == p, "the frames in front of the table are not the plain entry's"
    assert s[len(p):] == table_of(offs, prefixes(pre)), "the table is not LizardGPU_seekTableWrite of the offsets"
    table = a.stream_seek_table_device(device(s))
    assert [(e["offset"], e["decoded_bytes"], e["prefix_bytes"]) for e in table] == [(offs[i], SIZES[i], len(prefixes(pre)[i]) if pre else 0)
                                                                                      for i in range(len(SIZES))]
    assert sum(e["prefix_bytes"] + e["frame_bytes"] for e in table) == len(p)
    assert a.stream_seek_table_device(a.compress_stream_device_into(tensors(), level=level, block_size_id=1)[0]) is None


@pytest.mark.parametrize("chunk", (1, 3))
def test_offsets_across_a_chunk_carry(chunk):
    a = api()
    for level, checksum, pre in ((10, 1, 1), (30, 0, 0)):
        p, s, offs = streams(level, checksum, pre)
        os.environ[CHUNK_ENV] = str(chunk)
        c0 = counters("LizardGPU_streamCompressDeviceStats")
        got, goffs = a.compress_stream_device_into(tensors(), prefixes=prefixes(pre), level=level, block_size_id=1, checksum=bool(checksum), seekable=True)
        c1 = counters("LizardGPU_streamCompressDeviceStats")
        os.environ.pop(CHUNK_ENV)
        assert c1[2] - c0[2] == -(-8 // chunk) and c1[3] - c0[3] == 1 and c1[0] - c0[0] == len(SIZES)
        assert host(got) == s and tuple(goffs) == offs, (level, checksum, pre, chunk)


def guarded(cap):
    import torch
    whole = torch.full((cap + 2 * G,), CANARY, dtype=torch.uint8, device="cuda")
    return whole, whole[G:G + cap]


@pytest.mark.parametrize("pre", (0, 1))
def test_capacity_exact_one_below_and_the_bound(pre):
    from lizard_amd import _lib
    a, L = api(), lib()
    p, s, offs = streams(10, 1, pre)
    n = len(SIZES)
    prefs = util.frame_prefs(10, 1, 1, 1, 1)
    pre_sizes = (C.c_size_t * n)(*[len(x) for x in prefixes(pre)]) if pre else None
    bound = L.LizardGPU_compressStreamBound(n, (C.c_size_t * n)(*SIZES), pre_sizes, C.byref(prefs)) + L.LizardGPU_seekTableBytes(n)
    for cap in (len(s), bound):
        whole, dst = guarded(cap)
        got, _ = a.compress_stream_device_into(tensors(), dst=dst, prefixes=prefixes(pre), level=10, block_size_id=1, checksum=True, seekable=True)
        assert got.data_ptr() == dst.data_ptr() and host(got) == s
        w = whole.cpu().numpy()
        assert (w[:G] == CANARY).all() and (w[G + cap:] == CANARY).all(), "written outside d_dst"
    for cap in (len(s) - 1, len(p), len(p) - 1, si.table_bytes(n) - 1):      # the table's last byte / the whole table / a frame's byte / nothing fits
        whole, dst = guarded(cap)
        with pytest.raises(_lib.LizardAmdError, match="dstMaxSize_tooSmall"):
            a.compress_stream_device_into(tensors(), dst=dst, prefixes=prefixes(pre), level=10, block_size_id=1, checksum=True, seekable=True)
        w = whole.cpu().numpy()
        assert (w[:G] == CANARY).all() and (w[G + cap:] == CANARY).all(), ("written outside d_dst", cap)
    out = a.compress_stream_device_into(tensors(), prefixes=prefixes(pre), level=10, block_size_id=1, checksum=True, seekable=True)[0]
    assert out.untyped_storage().nbytes() == bound and out.numel() == len(s)


# ---- reader identity ----

def decode(name, stream, cap, flags=0):
    """One of the two whole-stream entries on `stream` (bytes) into a guarded buffer of cap bytes: (error, result, consumed, frames,
    decoded, the decoded bytes)."""
    import torch
    L = lib()
    src = device(stream)
    whole, dst = guarded(cap)
    used, frames, decoded = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
    r = getattr(L, name)(dst.data_ptr(), cap, src.data_ptr(), len(stream), C.byref(used), C.byref(frames), C.byref(decoded), flags,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    w = whole.cpu().numpy()
    assert (w[:G] == CANARY).all() and (w[G + cap:] == CANARY).all(), (name, "written outside d_dst")
    return err(r), 0 if err(r) else r, used.value, frames.value, decoded.value, w[G:G + decoded.value].tobytes()


def both(stream, cap, flags=0):
    """(the walking entry's answer, the seekable entry's answer, growth of LizardGPU_seekDeviceStats)"""
    want = decode("LizardGPU_decompressStream_device", stream, cap, flags)
    c0 = counters()
    got = decode("LizardGPU_decompressSeekableStream_device", stream, cap, flags)
    return want, got, [y - x for x, y in zip(c0, counters())]


@pytest.mark.parametrize("pre", (0, 1))
@pytest.mark.parametrize("level,checksum", ((10, 0), (10, 1), (30, 1)))
def test_an_intact_stream_is_answered_through_the_table(level, checksum, pre):
    p, s, offs = streams(level, checksum, pre)
    total = sum(SIZES)
    n_frames = len(SIZES) + (len(SIZES) - 1 if pre else 0) + 1
    for cap, flags in ((total, 0), (total + 1000, 1)):
        want, got, grown = both(s, cap, flags)
        assert want == got == (0, total, len(s), n_frames, total, b"".join(plain())), (cap, want[:5], got[:5])
        assert grown == [1, 0, 0, 1], grown
    for cap in (total - 1, 0):                                  # the sum does not fit: the walk's answer, whatever it is
        want, got, grown = both(s, cap)
        assert want == got and want[0] == E_TOO_SMALL, (cap, want[:5], got[:5])
        assert grown[:2] == [0, 1], grown
    # a stream without a table: the walk
    want, got, grown = both(p, total)
    assert want == got == (0, total, len(p), n_frames - 1, total, b"".join(plain())) and grown == [0, 1, 0, 0]


@pytest.mark.parametrize("pre", (0, 1))
def test_damaged_and_lying_tables_answer_like_the_walk(pre):
    p, s, offs = streams(10, 1, pre)
    total = sum(SIZES)
    for name, bad in si.damaged(s) + si.lying(s):
        for cap in (total, total - 1, 0) if name.startswith(("the tag", "entry 1 decodes", "two")) else (total,):
            cap = 2 * total if name.startswith("two") and cap == total else cap
            want, got, grown = both(bad, cap)
            assert want == got, (name, cap, want[:5], got[:5])
            assert grown[:2] == [0, 1], (name, cap, grown)


def test_a_damaged_frame_gives_the_walks_error_and_offset():
    for pre in (0, 1):
        p, s, offs = streams(10, 1, pre)
        at = offs[4] + (len(prefixes(pre)[4]) if pre else 0) + 15 + 4 + 100      # a payload byte of the 131 073-byte frame's first block
        bad = s[:at] + bytes([s[at] ^ 0x40]) + s[at + 1:]
        want, got, grown = both(bad, sum(SIZES))
        assert want == got and want[0] and want[2] == offs[4] + (len(prefixes(pre)[4]) if pre else 0), (want[:5], got[:5])
        assert want[4] == sum(SIZES[:4]) and grown[:2] == [0, 1]


def test_null_arguments_and_the_empty_stream_answer_like_the_walk():
    L = lib()
    a, b, c = C.c_size_t(7), C.c_size_t(8), C.c_size_t(9)
    assert L.LizardGPU_decompressSeekableStream_device(None, 0, None, 0, C.byref(a), C.byref(b), C.byref(c), 0, None) == 0
    assert (a.value, b.value, c.value) == (7, 8, 9), "srcSize == 0 touches nothing"
    assert err(L.LizardGPU_decompressSeekableStream_device(None, 5, None, 10, C.byref(a), None, None, 0, None)) == E_GENERIC and a.value == 0


# ---- items ----

def items_call(stream, items, cap=None):
    """LizardGPU_decompressStreamItems_device on `stream` (bytes): (error, result, failedItem, itemOffsets, the bytes)."""
    import torch
    L = lib()
    src = device(stream)
    cap = sum(SIZES) if cap is None else cap
    whole, dst = guarded(cap)
    n = len(items)
    offs, failed = (C.c_uint64 * (n + 1))(*([77] * (n + 1))), C.c_size_t(99)
    r = L.LizardGPU_decompressStreamItems_device(dst.data_ptr(), cap, src.data_ptr(), len(stream), (C.c_size_t * max(n, 1))(*items), n, offs, C.byref(failed), 0,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    w = whole.cpu().numpy()
    assert (w[:G] == CANARY).all() and (w[G + cap:] == CANARY).all(), "written outside d_dst"
    return err(r), 0 if err(r) else r, failed.value, list(offs), w[G:G + (0 if err(r) else r)].tobytes(), w[G:G + cap]


@pytest.mark.parametrize("pre", (0, 1))
def test_items_some_all_and_none(pre):
    p, s, offs = streams(10, 1, pre)
    n = len(SIZES)
    for items in ([0], [n - 1], [1, 3], list(range(n)), [2, 4, 5]):
        c0 = counters()
        e, r, failed, ioffs, data, _ = items_call(s, items)
        assert (e, r, failed) == (0, sum(SIZES[k] for k in items), 99), (items, e)
        assert data == b"".join(plain()[k] for k in items), items
        assert ioffs == [sum(SIZES[k] for k in items[:j]) for j in range(len(items) + 1)]
        assert [y - x for x, y in zip(c0, counters())] == [0, 0, len(items), 1]
    e, r, failed, ioffs, data, buf = items_call(s, [])
    assert (e, r, failed, ioffs) == (0, 0, 99, [77]) and (buf == CANARY).all(), "nItems == 0 touches nothing"
    views = api().decompress_stream_items_device(device(s), [1, 3])
    assert [host(v) for v in views] == [plain()[1], plain()[3]]


def test_items_refusals():
    from lizard_amd import _lib
    p, s, offs = streams(10, 1, 1)
    n = len(SIZES)
    for items, code, failed in (([n], E_SIZE, 0), ([0, 1, n + 5], E_SIZE, 2), ([3, 1], E_BLOCK_MODE, 1), ([2, 2], E_BLOCK_MODE, 1)):
        e, r, f, _, _, buf = items_call(s, items)
        assert (e, f) == (code, failed) and (buf == CANARY).all(), (items, e, f)
    for name, stream in [("no table", p)] + si.damaged(s)[:3]:
        e, r, f, _, _, buf = items_call(stream, [0, 1])
        assert e == E_TYPE and (buf == CANARY).all(), (name, e)
    e, r, f, _, _, buf = items_call(s, [4, 5], cap=SIZES[4] + SIZES[5] - 1)
    assert e == E_TOO_SMALL and (buf == CANARY).all()
    # the table locates, the decoder validates: an item whose frame is damaged, or does not answer its entry, is that item's error
    at = offs[4] + len(prefixes(1)[4]) + 15 + 4 + 100
    bad = s[:at] + bytes([s[at] ^ 0x40]) + s[at + 1:]
    e, r, f, _, _, _ = items_call(bad, [1, 4, 5])
    assert e and f == 1
    e, r, f, _, data, _ = items_call(bad, [1, 3, 5])
    assert (e, data) == (0, plain()[1] + plain()[3] + plain()[5]), "an item that was not asked for cannot fail the call"
    lies = dict(si.lying(s))
    e, r, f, _, _, _ = items_call(lies["entry 1 decodes to one byte more"], [0, 1, 2])
    assert e and f == 1
    e, r, f, _, _, _ = items_call(lies["two seekable streams back to back"], [n - 1], cap=2 * sum(SIZES))
    assert e and f == 0, "the last item of a concatenation's table does not fill its region"
    with pytest.raises(_lib.LizardAmdError, match="frameType_unknown"):
        api().decompress_stream_items_device(device(p), [0])


# ---- tensor streams ----

@functools.lru_cache(maxsize=None)
def host_tensors():
    import torch
    g = torch.Generator().manual_seed(5)
    return ((torch.randn(1000, 37, generator=g) * 0.02).to(torch.bfloat16), torch.randn(70001, generator=g),
            torch.randint(0, 256, (5,), generator=g).to(torch.uint8), torch.tensor(True), torch.empty(0, 3, dtype=torch.float16),
            (torch.randn(300, 11, generator=g) * 0.02).to(torch.bfloat16))


def same(back, want):
    import torch
    assert len(back) == len(want)
    for b, t in zip(back, want):
        assert b.is_cuda and b.dtype == t.dtype and tuple(b.shape) == tuple(t.shape)
        assert torch.equal(b.cpu().reshape(-1).view(torch.uint8), t.contiguous().reshape(-1).view(torch.uint8)), (t.dtype, tuple(t.shape))


@pytest.mark.parametrize("planes", ("bytes", "bits"))
def test_tensor_streams(planes):
    import torch
    from lizard_amd import _lib
    a = api()
    want = host_tensors()
    dev = [t.cuda() for t in want]
    base = [None] * len(dev)
    base[5] = (want[5].float() * 1.001).to(torch.bfloat16).cuda()                # an earlier version of tensor 5
    kw = dict(level=10, checksum=True, planes=planes, base=base, base_tag=41)
    before = a.compress_tensors_device(dev, **kw)
    stream = a.compress_tensors_device(dev, seekable=True, **kw)
    n = before.numel()
    assert host(stream[:n]) == host(before) and stream.numel() == n + si.table_bytes(len(dev)), "seekable=False is what it was; seekable adds the table"
    table = a.stream_seek_table_device(stream)
    assert [e["decoded_bytes"] for e in table] == [t.numel() * t.element_size() for t in want]
    assert [e["prefix_bytes"] for e in table] == [i["header_bytes"] for i in a.tensors_info_device(before)]
    assert a.tensors_info_device(stream) == a.tensors_info_device(before) == a.tensors_info_device(stream, seek=True)
    walk0, seek0 = counters("LizardGPU_streamDecodeDeviceStats"), counters()
    same(a.decompress_tensors_device(stream, base=base, base_tag=41, seek=True), want)
    assert counters("LizardGPU_streamDecodeDeviceStats") == walk0, "seek=True walked the stream"
    assert [y - x for x, y in zip(seek0, counters())][:2] == [1, 0]
    same(a.decompress_tensors_device(stream, base=base, base_tag=41), want)                       # the old path steps over the table
    same(a.decompress_tensors_device(before, base=base, base_tag=41), want)
    for select in ([0], [5], [1, 3], [2, 3, 4, 5], list(range(len(want)))):
        seek0 = counters()
        same(a.decompress_tensors_device(stream, base=base, base_tag=41, select=select), [want[k] for k in select])
        assert [y - x for x, y in zip(seek0, counters())][:3] == [0, 0, len(select)]
    assert a.decompress_tensors_device(stream, base=base, select=[]) == []
    for bad in ([6], [3, 1], [2, 2]):
        with pytest.raises(_lib.LizardAmdError):
            a.decompress_tensors_device(stream, base=base, select=bad)
    for kwargs in (dict(seek=True), dict(select=[0])):
        with pytest.raises(_lib.LizardAmdError, match="seek table"):
            a.decompress_tensors_device(before, base=base, **kwargs)
    with pytest.raises(_lib.LizardAmdError, match="seek table"):
        a.tensors_info_device(before, seek=True)
    with pytest.raises(_lib.LizardAmdError, match="no base|none was given"):
        a.decompress_tensors_device(stream, select=[5])


def test_plain_streams_through_the_python_entries():
    import torch
    a = api()
    p, s, offs = streams(30, 0, 0)
    dev = device(s)
    assert host(a.compress_stream_device(tensors(), level=30, block_size_id=1, seekable=True)) == s
    assert host(a.compress_stream_device(tensors(), level=30, block_size_id=1)) == p
    for seek in (False, True):
        back, frames = a.decompress_stream_device(dev, seek=seek)
        assert host(back) == b"".join(plain()) and frames == len(SIZES) + 1
    back, frames = a.decompress_stream_device(device(p), seek=True)
    assert host(back) == b"".join(plain()) and frames == len(SIZES)


# ---- the reference's CLI ----

@pytest.mark.parametrize("pre", (0, 1))
def test_the_reference_cli_decodes_a_seekable_file_to_the_payloads(pre, tmp_path):
    exe = os.path.join(util.ROOT, "oracle", "_ref", "lizard_cli_ref")
    if not os.path.exists(exe):
        util.need_ref("oracle/_ref/lizard_cli_ref")
    p, s, offs = streams(10, 1, pre)
    (tmp_path / "in.liz").write_bytes(s)
    r = subprocess.run([exe, "-d", "-f", str(tmp_path / "in.liz"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.bin").read_bytes() == b"".join(plain())
