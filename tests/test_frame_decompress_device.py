"""LizardGPU_decompressFrame_device / LizardGPU_frameIndex_device: frames that lie in device memory, decoded into device memory.
Every case also runs the host-memory twin LizardGPU_decompressFrame on the same bytes and requires the same result, consumed count
and bytes; source and destination are torch tensors with 4 KiB canary margins on both sides, checked after every call."""
import collections
import ctypes as C
import os
import random
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_frame_decompress_gpu as fd

pytestmark = pytest.mark.gpu

SEED = 20261017
G = 4096
CANARY = 0xC3
SKIP_CHECKSUM = 1
E_GENERIC, E_TOO_SMALL, E_CONTENT_CRC = 1, 11, 18
BS = util.FRAME_BLOCK_SIZES
SKIP = struct.pack("<II", 0x184D2A57, 9) + b"skippable"


def lib():
    from lizard_amd import _lib
    fd.lib()
    return _lib.lib()


def dstats():
    out = (C.c_ulonglong * 4)()
    assert lib().LizardGPU_frameDecodeDeviceStats(out) == 0
    return list(out)


def grown(s0):
    return [b - a for a, b in zip(s0, dstats())]


def padded(data, fill):
    """A CUDA tensor: 4 KiB of `fill`, the bytes, 4 KiB of `fill`."""
    import numpy as np
    import torch
    a = np.full(len(data) + 2 * G, fill, dtype=np.uint8)
    a[G:G + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    return torch.from_numpy(a).cuda()


def margins_intact(t, n, fill, what):
    h = t.cpu().numpy()
    assert (h[:G] == fill).all() and (h[G + n:] == fill).all(), what
    return h[G:G + n]


def device_only(frame, cap, flags=0):
    """(error number or 0, consumed, bytes) of the device entry."""
    import torch
    L = lib()
    src, dst = padded(frame, 0x5A), padded(bytes(cap), CANARY)
    dst[G:G + cap] = CANARY
    used = C.c_size_t(12345)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = L.LizardGPU_decompressFrame_device(dst.data_ptr() + G, cap, src.data_ptr() + G, len(frame), C.byref(used), flags, stream)
    body = margins_intact(dst, cap, CANARY, "the device frame decoder wrote outside d_dst")
    assert margins_intact(src, len(frame), 0x5A, "the source changed").tobytes() == bytes(frame)
    e = fi.err_of(r)
    if e:
        assert used.value == 0
        return e, 0, b""
    assert r <= cap
    return 0, used.value, body[:r].tobytes()


def both(frame, cap, flags=0):
    """The device entry and the host twin on the same bytes: identical, returned once."""
    got = device_only(frame, cap, flags)
    want = fd.gpu_decode(frame, cap)
    assert got == want, ("device entry and host twin disagree", got[:2], want[:2], cap, len(frame))
    return got


def check_frame(frame, plain, what):
    b = fi.bound(frame)
    assert not fi.err_of(b) and b >= len(plain), what
    caps = sorted({len(plain), b, len(plain) + 77})
    for cap in caps:
        e, used, got = both(frame, cap)
        assert (e, used) == (0, len(frame)) and got == plain, (what, cap, e)
    if len(plain):
        assert both(frame, len(plain) - 1)[0] == E_TOO_SMALL, what
    return len(caps) + (1 if len(plain) else 0)                 # calls of the device entry


def run_round_trips():
    data = dict(util.corpus())
    for name, case, level, bsid, checksum, csize in util.FRAME_CASES:
        for mode in (1, 0):
            frame, plain = fd.make_frame(data[case], level, bsid, checksum, csize, mode), data[case]
            n = fi.index(frame)[4]
            s0 = dstats()
            calls = check_frame(frame, plain, (name, mode))
            d = grown(s0)
            print(name, mode, n, calls, d)
            assert d[2] == 0, "a frame of this library was finished on the host"
            assert (d[0] > 0) == (n > 0), (name, d)
            if n and len(plain) % BS[frame[5] >> 4] == 0:
                assert d[1] == 0, ("a frame of full blocks went through staging", name, d)
            yield n, d, calls


def test_round_trips_of_the_frame_cases():
    assert len(list(run_round_trips())) == 2 * len(util.FRAME_CASES)


def flushed_case():
    data = util.datagen(600001, 0.5, 0.0, 61)
    head = [131072, 1, 70000, 131073, 262144 + 17, 5]
    return data, head + [len(data) - sum(head)]


def run_flushed():
    data, pieces = flushed_case()
    for mode in (1, 0):
        frame = fd.flushed_frame(data, pieces, mode=mode)
        assert fi.index(frame)[4] > len(pieces)
        s0 = dstats()
        calls = check_frame(frame, data, ("flushed", mode))
        d = grown(s0)
        assert d[1] > 0 and d[0] > 0 and d[2] == 0, d
        yield fi.index(frame)[4], d, calls


def test_short_blocks_in_the_middle_are_moved_into_place_on_the_device():
    assert len(list(run_flushed())) == 2


def test_raw_records():
    noise = dict(util.corpus())["random256k"]
    f_raw = fd.make_frame(noise, 10, 1, 1, 0, 1)
    assert all(w >> 31 for w in fi.index(f_raw)[3])
    s0 = dstats()
    check_frame(f_raw, noise, "all raw")
    assert grown(s0)[1:3] == [0, 0]
    flushed = fd.flushed_frame(noise[:250000], [100000, 131072, 18928], checksum=0)
    assert all(w >> 31 for w in fi.index(flushed)[3])
    s0 = dstats()
    check_frame(flushed, noise[:250000], "raw flushed")
    assert grown(s0)[1] > 0


def test_degenerate_and_concatenated_frames():
    import numpy as np
    import torch
    from lizard_amd import api
    data = dict(util.corpus())
    noise = data["random256k"]
    check_frame(fd.make_frame(b"x", 10, 1, 1, 0, 1), b"x", "one byte")
    for checksum in (0, 1):
        empty = fd.make_frame(b"", 10, 1, checksum, 0, 1)
        assert both(empty, 0) == (0, len(empty), b"") and both(empty, 100) == (0, len(empty), b"")
    assert both(SKIP, 0) == (0, len(SKIP), b"") and both(SKIP + b"tail", 50) == (0, len(SKIP), b"")
    assert both(SKIP[:-1], 50)[0] == E_GENERIC and both(SKIP[:7], 50)[0] == 12
    f1, f2 = fd.make_frame(data["text"], 21, 1, 1, 1, 1), fd.make_frame(data["alpha4"], 13, 1, 0, 0, 0)
    f_raw = fd.make_frame(noise, 10, 1, 1, 0, 1)
    stream = SKIP + f1 + f_raw + SKIP + f2
    pos, out = 0, []
    while pos < len(stream):
        e, used, got = both(stream[pos:], 1 << 19)
        assert e == 0 and used > 0
        out.append(got)
        pos += used
    assert out == [b"", data["text"], noise, b"", data["alpha4"]] and pos == len(stream)
    t = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    got = api.decompress_frame_device(t)
    assert got.is_cuda and got.cpu().numpy().tobytes() == data["text"] + noise + data["alpha4"]


def test_reference_made_golden_frames():
    for name, frame, plain, linked in fd.reference_frames():
        s0 = dstats()
        decodes = check_frame(frame, plain, name)
        d = grown(s0)
        if linked:
            assert d[2] == decodes, (name, d)
        else:
            assert d[2] == 0 and d[0] >= 10 and d[1] == 0, (name, d)


CHILD = r"""
import sys, os
import torch
assert torch.cuda.is_available()
sys.path.insert(0, os.path.join(%r, "tests"))
import test_frame_decompress_device as t
per_frame = []
for n, d, calls in list(t.run_round_trips()) + list(t.run_flushed()):
    assert d[3] == calls * (n // 2 + 1), (n, calls, d)          # two records per segment, and the segment that finds the end mark
    if n >= 2:
        assert d[3] > calls, (n, d)
        per_frame.append(d[3] / calls)
assert len(per_frame) > 10
print("segments per decode:", min(per_frame), max(per_frame))
print("ok")
"""


def test_many_segments_and_small_chunks():
    """LIZARDGPU_WALK_RECORDS=2 and LIZARDGPU_CHUNK_MB=1 in a fresh child process: every frame of two records or more is walked in
    more than one segment, and the staging path works in chunks."""
    env = dict(os.environ, LIZARDGPU_WALK_RECORDS="2", LIZARDGPU_CHUNK_MB="1")
    r = subprocess.run([sys.executable, "-c", CHILD % util.ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


def test_content_checksum_and_the_skip_flag():
    data = util.datagen(2 * 131072 + 500, 0.5, 0.0, 33)
    for mode in (1, 0):
        frame = fd.make_frame(data, 10, 1, 1, 0, mode)
        assert both(frame, len(data)) == (0, len(frame), data)
        assert device_only(frame, len(data), SKIP_CHECKSUM) == (0, len(frame), data)
        bad = frame[:-2] + bytes([frame[-2] ^ 0x10]) + frame[-1:]
        assert both(bad, len(data))[0] == E_CONTENT_CRC
        assert device_only(bad, len(data), SKIP_CHECKSUM) == (0, len(frame), data)
        for flags in (0, SKIP_CHECKSUM):
            assert device_only(frame[:-4], len(data), flags)[0] == E_GENERIC
            assert device_only(bad[:-1], len(data), flags)[0] == E_GENERIC
        assert both(frame[:-4], len(data))[0] == E_GENERIC
    # the reference's linked frame is finished on the host: the flag holds there too
    name, frame, plain, linked = fd.reference_frames()[0]
    assert linked and frame[4] & 4
    bad = frame[:-1] + bytes([frame[-1] ^ 1])
    assert both(bad, len(plain))[0] == E_CONTENT_CRC
    assert device_only(bad, len(plain), SKIP_CHECKSUM) == (0, len(frame), plain)


def big_checksummed_frame():
    """2 x 32 MiB + 12345 bytes, 256 KiB blocks, content checksum: three pieces of the checksum pass, the last one odd."""
    data = util.datagen(2 * (32 << 20) + 12345, 0.5, 0.0, 29)
    frame = fd.make_frame(data, 10, 2, 1, 0, 1)
    assert frame[4] & 4 and fi.index(frame)[4] == 257
    return data, frame


def run_checksum_pieces():
    data, frame = big_checksummed_frame()
    assert both(frame, len(data)) == (0, len(frame), data)
    bad = frame[:-1] + bytes([frame[-1] ^ 0x40])
    assert both(bad, len(data))[0] == E_CONTENT_CRC
    assert device_only(bad, len(data), SKIP_CHECKSUM) == (0, len(frame), data)


def test_content_checksum_in_three_pieces():
    """The D2H / XXH32 loop of the checksum pass with more than one piece at the product's piece size (32 MiB): piece i + 1 is copied
    into the other pinned buffer while piece i is hashed."""
    run_checksum_pieces()


PIECES_CHILD = r"""
import sys, os
import torch
assert torch.cuda.is_available()
sys.path.insert(0, os.path.join(%r, "tests"))
import test_frame_decompress_device as t
s0 = t.dstats()
t.run_checksum_pieces()
d = t.grown(s0)
assert d[3] == 3 * (257 // 64 + 1) and d[2] == 0, d             # 64 records per segment: 16 MiB of every segment are hashed while the next decodes
print("ok")
"""


def test_content_checksum_pieces_across_segments():
    """The same frame with LIZARDGPU_WALK_RECORDS=64 in a fresh child process: five segments, the pieces of a segment are copied and
    hashed while the next segment decodes."""
    env = dict(os.environ, LIZARDGPU_WALK_RECORDS="64")
    r = subprocess.run([sys.executable, "-c", PIECES_CHILD % util.ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


def device_index(frame, max_records=None):
    """fi.index through LizardGPU_frameIndex_device: (rc, info, offsets, words, nRecords, frameBytes)."""
    import torch
    L = lib()
    src = padded(frame, 0x5A)
    info = util.FrameInfo()
    n, fb = C.c_size_t(0), C.c_size_t(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.LizardGPU_frameIndex_device(src.data_ptr() + G, len(frame), C.byref(info), None, None, 0, C.byref(n), C.byref(fb), stream)
    if rc:
        return rc, info, [], [], n.value, fb.value
    m = n.value if max_records is None else max_records
    offs = torch.full((m + 2,), -7, dtype=torch.int64, device="cuda")
    words = torch.full((m + 2,), -7, dtype=torch.int32, device="cuda")
    rc = L.LizardGPU_frameIndex_device(src.data_ptr() + G, len(frame), C.byref(info), offs.data_ptr() + 8, words.data_ptr() + 4, m,
                                       C.byref(n), C.byref(fb), stream)
    o, w = offs.cpu().tolist(), [x & 0xFFFFFFFF for x in words.cpu().tolist()]
    k = min(m, n.value)
    assert o[0] == -7 and all(x == -7 for x in o[1 + k:]) and w[0] == 0xFFFFFFF9 and all(x == 0xFFFFFFF9 for x in w[1 + k:]), "the index wrote outside its tables"
    return rc, info, o[1:1 + k], w[1:1 + k], n.value, fb.value


def same_index(a, b):
    fields = lambda i: (i.blockSizeID, i.blockMode, i.contentChecksumFlag, i.frameType, i.contentSize)
    return (a[0], fields(a[1])) + tuple(a[2:]) == (b[0], fields(b[1])) + tuple(b[2:])


def test_frame_index_device_matches_the_host_walk():
    data = dict(util.corpus())
    frames = [fd.make_frame(data[case], level, bsid, checksum, csize, 1) for _, case, level, bsid, checksum, csize in util.FRAME_CASES]
    frames += [f for _, f in fd.intact_frames()] + [SKIP, SKIP + b"x"]
    d, pieces = flushed_case()
    frames.append(fd.flushed_frame(d, pieces))
    for f in frames:
        assert same_index(device_index(f), fi.index(f))
        assert same_index(device_index(f + b"\x04\x22\x4d\x18tail"), fi.index(f + b"\x04\x22\x4d\x18tail"))
    big = frames[-1]
    assert same_index(device_index(big, 3), fi.index(big, 3))
    rnd = random.Random(SEED)
    bases = fd.intact_frames()
    counts = collections.Counter()
    for i in range(300):
        kind, bad = fd.damage(rnd, bases[i % len(bases)][1])
        want = fi.index(bad)
        assert same_index(device_index(bad), want), (kind, i)
        counts[want[0]] += 1
    print(dict(counts))
    assert counts[0] > 15 and 300 - counts[0] > 15, counts


def test_differential_on_damaged_frames():
    """550 damaged frames: the device entry and the host twin agree on the error number, the consumed count and the bytes.  The
    streaming host decoder LizardF_decompress says which of them are valid frames at all."""
    rnd = random.Random(SEED)
    bases = fd.intact_frames()
    accepted = refused = total = 0
    kinds = collections.Counter()
    for i in range(550):
        name, frame = bases[i % len(bases)]
        kind, bad = fd.damage(rnd, frame)
        cap = fd.slot_bound(bad)
        total += 1
        e, used, got = both(bad, cap)
        he, hint, hused, hgot = fi.host_one_call(bad, cap)
        if he == 0 and hint == 0:
            accepted += 1
            assert (e, used, got) == (0, hused, hgot), (name, kind, i)
        else:
            refused += 1
        kinds[kind, e] += 1
    print("seed %d: %d accepted by the host decoder, %d refused" % (SEED, accepted, refused))
    for k in sorted(kinds):
        print("  %-14s error %-3d %d" % (k[0], k[1], kinds[k]))
    assert total == 550 and accepted > 5 and refused > 250


def test_python_interface():
    import numpy as np
    import torch
    from lizard_amd import api, _lib
    data = util.datagen(3 * 262144 + 1234, 0.5, 0.0, 13)
    frame = api.compress_frame(data, level=30, block_size_id=2, checksum=True, content_size=True)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        src = torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy()).cuda(non_blocking=True)
        info = api.frame_index_device(src)
        host = api.frame_info(frame)
        assert {k: info[k] for k in host} == host
        assert info["offsets"].is_cuda and info["words"].is_cuda and info["offsets"].numel() == info["n_records"] == 4
        assert info["offsets"].cpu().tolist() == fi.index(frame)[2]
        out = api.decompress_frame_device(src)
        assert out.device == src.device and out.dtype == torch.uint8 and out.cpu().numpy().tobytes() == data
        dst = torch.empty(len(data) + 100, dtype=torch.uint8, device="cuda")
        view = api.decompress_frame_device(src, dst)
        assert view.data_ptr() == dst.data_ptr() and view.cpu().numpy().tobytes() == data
        wrong = bytearray(frame); wrong[-1] ^= 1
        bad = torch.from_numpy(np.frombuffer(bytes(wrong), dtype=np.uint8).copy()).cuda()
        with pytest.raises(_lib.LizardAmdError):
            api.decompress_frame_device(bad)
        assert api.decompress_frame_device(bad, verify_checksum=False).cpu().numpy().tobytes() == data
        cut = torch.from_numpy(np.frombuffer(frame[:len(frame) // 2], dtype=np.uint8).copy()).cuda()
        with pytest.raises(_lib.LizardAmdError):
            api.decompress_frame_device(cut, verify_checksum=False)
    stream.synchronize()
