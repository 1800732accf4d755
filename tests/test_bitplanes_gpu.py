"""LizardGPU_splitBitPlanes_device / LizardGPU_joinBitPlanes_device on the GPU: the batch of tests/test_bitplanes_emul.py
(tests/bitplanes_inputs.py: every element size, every size at which the kernels take another path, src / dst offsets from a 16-byte
boundary in every pair, 300 one-byte buffers — under 12 MiB) in torch buffers, ONE launch each way.  Every dst equals the numpy model,
the 64 bytes of 0x5A around every dst are intact, join(split(x)) == x; every -LIZARDGPU_ERR_ARG case launches nothing and leaves dst
untouched; nBuffers == 0 works; LizardGPU_bitPlanesStats counts buffers, bytes and launches, and LizardGPU_planesStats — the byte
planes' — does not move."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bitplanes_inputs as bi

pytestmark = pytest.mark.gpu

ERR_ARG = 3


def lib():
    from lizard_amd import _lib
    return _lib.lib()


def stats():
    out = (C.c_ulonglong * 4)()
    assert lib().LizardGPU_bitPlanesStats(out) == 0
    return list(out)


def byte_stats():
    out = (C.c_ulonglong * 4)()
    assert lib().LizardGPU_planesStats(out) == 0
    return list(out)


def call(join, srcs, dsts, sizes, elems, n=None):
    import torch
    L = lib()
    fn = L.LizardGPU_joinBitPlanes_device if join else L.LizardGPU_splitBitPlanes_device
    k = len(sizes)
    arr = lambda t, v: None if v is None else (t * k)(*v)
    return fn(k if n is None else n, arr(C.c_void_p, dsts), arr(C.c_void_p, srcs), arr(C.c_size_t, sizes), arr(C.c_uint32, elems),
              C.c_void_p(torch.cuda.current_stream().cuda_stream))


def run(cases, src, s_at, d_total, d_at, join):
    """One call over the whole batch, the empty buffers included.  src: a uint8 CUDA tensor.  Returns the dst arena (CUDA)."""
    import torch
    dst = torch.full((d_total,), bi.FILL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    s0, b0 = stats(), byte_stats()
    rc = call(join, [src.data_ptr() + s for s in s_at], [dst.data_ptr() + d for d in d_at], [c[1] for c in cases], [c[0] for c in cases])
    assert rc == 0, (rc, lib().LizardGPU_lastError())
    grown = [b - a for a, b in zip(s0, stats())]
    assert grown == [0 if join else len(cases), len(cases) if join else 0, sum(c[1] for c in cases), 1], grown
    assert byte_stats() == b0, "a bit-plane call counted as a byte-plane call"
    return dst


def check(cases, dst, d_at, want):
    dst = dst.cpu().numpy()
    mask = np.ones(dst.size, dtype=bool)
    for i, ((E, size, so, do), d) in enumerate(zip(cases, d_at)):
        got = dst[d:d + size]
        assert np.array_equal(got, want(i)), ("buffer", i, "E", E, "size", size, "offsets", so, do,
                                              "first difference at", int(np.flatnonzero(got != want(i))[0]))
        mask[d:d + size] = False
    assert (dst[mask] == bi.FILL).all(), "a byte outside every dst changed"


@functools.lru_cache(maxsize=None)
def the_batch():
    cases = bi.batch()
    s_at, d_at, s_total, d_total = bi.place(cases)
    assert s_total + 3 * d_total < 12 << 20                      # the source and the three results of the test below
    keep = bi.source(s_total)
    return cases, s_at, d_at, s_total, d_total, keep, [bi.bits_split_model(keep[s:s + c[1]], c[0]) for c, s in zip(cases, s_at)]


def test_split_and_join_the_batch_against_the_numpy_model():
    import torch
    cases, s_at, d_at, s_total, d_total, keep, models = the_batch()
    src = torch.from_numpy(keep.copy()).cuda()
    planar = run(cases, src, s_at, d_total, d_at, False)
    check(cases, planar, d_at, lambda i: models[i])
    assert np.array_equal(src.cpu().numpy(), keep), "the source changed"
    joined = run(cases, src, s_at, d_total, d_at, True)
    check(cases, joined, d_at, lambda i: bi.bits_join_model(keep[s_at[i]:s_at[i] + cases[i][1]], cases[i][0]))
    back_cases = [(E, size, do, so) for E, size, so, do in cases]
    _, b_at, _, b_total = bi.place(back_cases)
    back = run(back_cases, planar, d_at, b_total, b_at, True)
    check(back_cases, back, b_at, lambda i: keep[s_at[i]:s_at[i] + cases[i][1]])


def test_every_bad_argument_launches_nothing_and_no_buffers_is_fine():
    import torch
    L = lib()
    n, size = 3, 4096
    src = torch.arange(n * size, dtype=torch.int32, device="cuda").to(torch.uint8)
    dst = torch.full((n * size,), bi.FILL, dtype=torch.uint8, device="cuda")
    srcs, dsts = [src.data_ptr() + i * size for i in range(n)], [dst.data_ptr() + i * size for i in range(n)]
    sizes, elems = [size] * n, [2, 4, 8]
    null_at = lambda v, i: v[:i] + [None] + v[i + 1:]
    bad = {
        "no dsts": (srcs, None, sizes, elems), "no srcs": (None, dsts, sizes, elems), "no sizes": (srcs, dsts, None, elems),
        "no element sizes": (srcs, dsts, sizes, None),
        "element size 0": (srcs, dsts, sizes, [2, 0, 8]), "element size 3": (srcs, dsts, sizes, [2, 4, 3]),
        "element size 16": (srcs, dsts, sizes, [16, 4, 8]),
        "a null src": (null_at(srcs, 2), dsts, sizes, elems), "a null dst": (srcs, null_at(dsts, 1), sizes, elems),
        "2^32 tiles": (srcs, dsts, [size, size, (1 << 32) * bi.TILE - 2 * bi.TILE], elems),
    }
    b0 = byte_stats()
    for join in (False, True):
        for what, (s, d, z, e) in bad.items():
            s0 = stats()
            if z is None:                                        # (the helper sizes its arrays by `sizes`)
                fn = L.LizardGPU_joinBitPlanes_device if join else L.LizardGPU_splitBitPlanes_device
                rc = fn(n, (C.c_void_p * n)(*d), (C.c_void_p * n)(*s), None, (C.c_uint32 * n)(*e), None)
            else:
                rc = call(join, s, d, z, e)
            assert rc == -ERR_ARG, (what, rc)
            assert L.LizardGPU_lastError() != b"", what
            assert stats() == s0, what
            torch.cuda.synchronize()
            assert bool((dst == bi.FILL).all()), (what, "dst changed")
        # no buffers: 0, with or without arrays, nothing touched
        s0 = stats()
        assert call(join, srcs, dsts, sizes, elems, n=0) == 0 and call(join, None, None, [], None, n=0) == 0
        assert stats() == s0 and bool((dst == bi.FILL).all())
        # empty entries are skipped, their pointers may be null; a batch of nothing else launches nothing
        assert call(join, [None, None], [None, None], [0, 0], [2, 8]) == 0
        assert stats() == s0
        assert call(join, [None, srcs[1]], [None, dsts[1]], [0, size], [4, 4]) == 0
        assert [b - a for a, b in zip(s0, stats())] == [0 if join else 2, 2 if join else 0, size, 1]
        got = dst.cpu().numpy()
        want = (bi.bits_join_model if join else bi.bits_split_model)(src.cpu().numpy()[size:2 * size], 4)
        assert (got[:size] == bi.FILL).all() and (got[2 * size:] == bi.FILL).all() and np.array_equal(got[size:2 * size], want)
        dst.fill_(bi.FILL)
    assert byte_stats() == b0


def test_the_python_twins_one_launch_each_and_aligned_views():
    import torch
    from lizard_amd import api
    g = torch.Generator().manual_seed(7)
    host = [torch.randn(1000, 37, generator=g).to(torch.bfloat16), torch.randint(0, 255, (4099,), generator=g).to(torch.uint8),
            torch.empty(0, dtype=torch.float32), torch.randn(515, generator=g, dtype=torch.float64)]
    elems = [2, 1, 4, 8]
    raw = [t.reshape(-1).view(torch.uint8).numpy() for t in host]
    s0 = stats()
    planar = api.split_bit_planes_device([t.cuda() for t in host])
    assert [b - a for a, b in zip(s0, stats())] == [len(host), 0, sum(r.size for r in raw), 1]
    assert all(p.dtype == torch.uint8 and (p.data_ptr() % 256 == 0 or not p.numel()) for p in planar)
    for p, r, E in zip(planar, raw, elems):
        assert np.array_equal(p.cpu().numpy(), bi.bits_split_model(r, E)), E
    s0 = stats()
    back = api.join_bit_planes_device(planar, elems)
    assert [b - a for a, b in zip(s0, stats())] == [0, len(host), sum(r.size for r in raw), 1]
    assert all(np.array_equal(b.cpu().numpy(), r) for b, r in zip(back, raw))
