"""GPU: paths of LizardGPU_decompressFrame that tests/test_frame_decompress_gpu.py does not reach — a source in pinned host memory
(the DMA reads the caller's buffer), callers on many threads mixed with compression and LizardGPU_shutdown, the smallest memory
budget (chunks shrink), and decode launches on one stream while compress launches on another share the context's arena."""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_frame_index as fi
import test_frame_decompress_gpu as tg
from golden.make_frame_golden import golden_frame_input

pytestmark = pytest.mark.gpu


def decode_pinned(frame, plain, offset):
    """The frame in pinned host memory `offset` bytes into the allocation; the decoded bytes must be `plain`."""
    import torch
    L = tg.lib()
    src = torch.empty(len(frame) + offset + 64, dtype=torch.uint8).pin_memory()
    src.fill_(0x5A)
    src[offset:offset + len(frame)] = torch.from_numpy(np.frombuffer(frame, dtype=np.uint8).copy())
    out = np.full(len(plain) + 128, tg.CANARY, dtype=np.uint8)
    used = C.c_size_t(0)
    r = L.LizardGPU_decompressFrame(out.ctypes.data + 64, len(plain), src.data_ptr() + offset, len(frame), C.byref(used))
    assert not fi.err_of(r), (fi.err_of(r), L.LizardGPU_lastError())
    assert (r, used.value) == (len(plain), len(frame))
    assert out[64:64 + r].tobytes() == plain
    assert (out[:64] == tg.CANARY).all() and (out[64 + r:] == tg.CANARY).all(), "the frame decoder wrote outside dst"


def pinned_cases(n):
    data = util.datagen(n, 0.5, 0.0, 23)
    for mode in (1, 0):
        frame = tg.make_frame(data, 10, 1, 1, 1, mode)
        for offset in (0, 7):
            decode_pinned(frame, data, offset)
    plain = golden_frame_input()
    for name in ("frame_ref_linked.liz", "frame_ref_independent.liz"):
        frame = open(os.path.join(util.GOLDEN_DIR, name), "rb").read()
        for offset in (0, 1):
            decode_pinned(frame, plain, offset)


def test_pinned_source_one_chunk():
    pinned_cases(3 * 131072 + 4321)


PINNED_CHILD = r"""
import sys, os
import torch
assert torch.cuda.is_available()        # torch's HIP runtime first, as in the test process: the library then shares it
sys.path.insert(0, os.path.join(%r, "tests"))
import test_frame_paths_gpu as t
t.pinned_cases((6 << 20) + 999)
print("ok")
"""


def test_pinned_source_many_chunks():
    env = dict(os.environ, LIZARDGPU_CHUNK_MB="1")
    r = subprocess.run([sys.executable, "-c", PINNED_CHILD % util.ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_threads_mixing_frame_decodes_compression_and_shutdown():
    from lizard_amd import api
    L = tg.lib()
    L.Lizard_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.LizardGPU_decompress_safe.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    data = util.datagen(5 * 131072 + 777, 0.5, 0.0, 31)
    bs = 131072
    blocks = [data[i:i + bs] for i in range(0, len(data), bs)]
    want = [util.oracle_compress(b, 10) for b in blocks]
    frames = [(tg.make_frame(data, 10, 1, 1, 1, 1), data), (tg.make_frame(data, 21, 1, 1, 0, 0), data),
              (open(os.path.join(util.GOLDEN_DIR, "frame_ref_linked.liz"), "rb").read(), golden_frame_input())]
    offsets = (C.c_uint64 * (len(want) + 1))()
    for i, w in enumerate(want):
        offsets[i + 1] = offsets[i] + len(w)
    blob = b"".join(want)
    stop = threading.Event()
    bad, calls = [], [0] * 12

    def worker(t):
        k = t
        while not stop.is_set() and not bad:
            kind = k % 5
            k += 1
            good = False
            try:
                good = one_call(kind, k)
            except Exception as e:                          # (an exception in a thread would otherwise pass for success)
                bad.append((t, kind, repr(e)))
            calls[t] += 1
            if not good:
                bad.append((t, kind, calls[t]))

    def one_call(kind, k):
        if kind == 0:
            frame, plain = frames[(k // 5) % 3]
            out = C.create_string_buffer(len(plain))
            used = C.c_size_t(0)
            r = L.LizardGPU_decompressFrame(out, len(plain), frame, len(frame), C.byref(used))
            good = r == len(plain) and used.value == len(frame) and out.raw == plain
        elif kind == 1:
            out = C.create_string_buffer(bs)
            i = (k // 5) % len(want)
            good = L.LizardGPU_decompress_safe(want[i], out, len(want[i]), bs) == len(blocks[i]) and out.raw[:len(blocks[i])] == blocks[i]
        elif kind == 2:
            out = C.create_string_buffer(len(want) * bs)
            sizes = (C.c_uint32 * len(want))()
            good = L.LizardGPU_decompressBlocks_host(blob, offsets, len(want), out, bs, sizes) == 0 and \
                b"".join(out.raw[i * bs:i * bs + sizes[i]] for i in range(len(want))) == data
        elif kind == 3:
            out = C.create_string_buffer(2 * bs)
            r = L.Lizard_compress(blocks[0], out, bs, 2 * bs, 10)
            good = out.raw[:max(r, 0)] == want[0]
        else:
            good = api.compress_blocks(data, bs, 10) == want
        return good

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(12)]
    for th in threads:
        th.start()
    for _ in range(4):
        time.sleep(4)
        L.LizardGPU_shutdown()
    time.sleep(4)
    stop.set()
    for th in threads:
        th.join(120)
        assert not th.is_alive(), "a caller hangs"
    assert not bad, bad
    assert min(calls) > 5, calls


def test_frames_at_the_smallest_memory_budget():
    L = tg.lib()
    L.LizardGPU_setMemoryBudget.argtypes = [C.c_size_t]; L.LizardGPU_setMemoryBudget.restype = C.c_int
    L.LizardGPU_memoryInUse.restype = C.c_size_t
    L.LizardGPU_residentWaves.restype = C.c_int
    data = b"".join(util.datagen(4 << 20, 0.5, 0.0, 700 + i) for i in range(25)) + util.datagen(12345, 0.5, 0.0, 9)
    frames = [tg.make_frame(data, 10, bsid, 1, 1, 1) for bsid in (2, 4)]
    cus = L.LizardGPU_residentWaves() // 13
    floor = cus * 16 * 5 * (131072 + 32) + (256 << 20)      # tests/test_memory_budget.py: one scratch arena + 256 MiB
    try:
        assert L.LizardGPU_setMemoryBudget(floor - 1) < 0
        assert L.LizardGPU_setMemoryBudget(floor) == 0
        for frame in frames:
            e, used, got = tg.gpu_decode(frame, len(data))
            assert (e, used) == (0, len(frame)), (e, L.LizardGPU_lastError())
            assert got == data
            assert 0 < L.LizardGPU_memoryInUse() <= floor
    finally:
        assert L.LizardGPU_setMemoryBudget(0) == 0


def test_decode_and_compress_launches_on_two_streams():
    import torch
    from lizard_amd import api
    bs = 262144
    data = [util.datagen(24 * bs + 1000 * i + 5, 0.5, 0.0, 50 + i) for i in range(3)]
    want = [[util.oracle_compress(d[o:o + bs], 10) for o in range(0, len(d), bs)] for d in data]
    frame = api.compress_frame(data[0], 21, 2, True, True)
    src = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in data]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        earlier = api.compress_blocks_device(src[0], bs, 10)
    torch.cuda.synchronize()
    comp, dec, framed = [], [], []
    for i in range(6):                                      # no host synchronisation between the launches of the two streams
        with torch.cuda.stream(sa):
            comp.append(api.compress_blocks_device(src[i % 3], bs, 10))
        with torch.cuda.stream(sb):
            dec.append(api.decompress_blocks_device(earlier[0], earlier[1], earlier[2], bs))
        if i % 2:
            framed.append(api.decompress_frame(frame))
    torch.cuda.synchronize()
    for i, (dst, sizes, stride) in enumerate(comp):
        out, sz = dst.cpu().numpy(), sizes.cpu().numpy()
        w = want[i % 3]
        assert list(sz) == [len(x) for x in w], i
        assert all(out[b * stride:b * stride + sz[b]].tobytes() == w[b] for b in range(len(w))), i
    for dst, out_sizes in dec:
        n = out_sizes.cpu().numpy()
        assert list(n) == [bs] * 24 + [5]
        assert dst.cpu().numpy()[:len(data[0])].tobytes() == data[0]
    assert framed == [data[0]] * 3
