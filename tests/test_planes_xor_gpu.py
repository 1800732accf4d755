"""LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device on the GPU: the batches of tests/test_planes_xor_emul.py (the
batches of tests/planes_inputs.py / tests/bitplanes_inputs.py, every buffer's base at its own offset from a 16-byte boundary, about
every fifth buffer without a base) in torch buffers, ONE launch each way, under 40 MiB in all.  Every dst equals the numpy model of
split(src ^ base) / join(src) ^ base, the 64 bytes of 0x5A around every dst are intact, src and base are unchanged,
join(split(x, b), b) == x; d_bases == NULL equals the plain entries' output byte for byte; every -LIZARDGPU_ERR_ARG case, a bad
filter included, launches nothing and changes no statistic and no dst; nBuffers == 0 and empty entries with null pointers work;
LizardGPU_planesXorStats grows by the call's buffers, bytes and one launch while LizardGPU_planesStats / LizardGPU_bitPlanesStats
do not move."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planes_inputs as pi
import bitplanes_inputs as bi
from planes_xor_inputs import base_offsets, place_bases

pytestmark = pytest.mark.gpu

ERR_ARG = 3
BYTES, BITS = 0, 1
FILTERS = {"bytes": (BYTES, pi, pi.split_model, pi.join_model), "bits": (BITS, bi, bi.bits_split_model, bi.bits_join_model)}


def lib():
    from lizard_amd import _lib
    return _lib.lib()


def stats(name="LizardGPU_planesXorStats"):
    out = (C.c_ulonglong * 4)()
    assert getattr(lib(), name)(out) == 0
    return list(out)


def plain_stats():
    return stats("LizardGPU_planesStats") + stats("LizardGPU_bitPlanesStats")


def call(join, srcs, dsts, bases, sizes, elems, filt, n=None):
    import torch
    L = lib()
    fn = L.LizardGPU_joinPlanesXor_device if join else L.LizardGPU_splitPlanesXor_device
    k = len(sizes)
    arr = lambda t, v: None if v is None else (t * k)(*v)
    return fn(k if n is None else n, arr(C.c_void_p, dsts), arr(C.c_void_p, srcs), arr(C.c_void_p, bases), arr(C.c_size_t, sizes),
              arr(C.c_uint32, elems), filt, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def run(mod, filt, cases, src, s_at, base, b_at, d_total, d_at, join):
    """One call over the whole batch, the empty buffers included.  src, base: uint8 CUDA tensors (base None: d_bases == NULL).
    Returns the dst arena (CUDA)."""
    import torch
    dst = torch.full((d_total,), mod.FILL, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and (base is None or base.data_ptr() % 16 == 0)
    s0, p0 = stats(), plain_stats()
    bases = None if base is None else [None if b is None else base.data_ptr() + b for b in b_at]
    rc = call(join, [src.data_ptr() + s for s in s_at], [dst.data_ptr() + d for d in d_at], bases, [c[1] for c in cases], [c[0] for c in cases], filt)
    assert rc == 0, (rc, lib().LizardGPU_lastError())
    grown = [b - a for a, b in zip(s0, stats())]
    assert grown == [0 if join else len(cases), len(cases) if join else 0, sum(c[1] for c in cases), 1], grown
    assert plain_stats() == p0, "a plain entry's statistics moved"
    return dst


def check(mod, cases, dst, d_at, want):
    dst = dst.cpu().numpy()
    mask = np.ones(dst.size, dtype=bool)
    for i, ((E, size, so, do), d) in enumerate(zip(cases, d_at)):
        got, w = dst[d:d + size], want(i)
        assert np.array_equal(got, w), ("buffer", i, "E", E, "size", size, "offsets", so, do,
                                        "first difference at", int(np.flatnonzero(got != w)[0]))
        mask[d:d + size] = False
    assert (dst[mask] == mod.FILL).all(), "a byte outside every dst changed"


@functools.lru_cache(maxsize=None)
def the_batch(planes):
    mod = FILTERS[planes][1]
    cases = mod.batch()
    s_at, d_at, s_total, d_total = mod.place(cases)
    b_off = base_offsets(cases, list(mod.OFFSETS))
    b_at, b_total = place_bases(cases, b_off)
    assert 2 * (s_total + b_total + 5 * d_total) < 40 << 20     # both filters: source, bases, and the results alive in one test
    return cases, s_at, d_at, s_total, d_total, b_at, mod.source(s_total), mod.source(b_total, seed=6)


@pytest.mark.parametrize("planes", ["bytes", "bits"])
def test_split_and_join_the_batch_with_bases_against_the_numpy_model(planes):
    import torch
    filt, mod, split_model, join_model = FILTERS[planes]
    cases, s_at, d_at, s_total, d_total, b_at, keep, keep_base = the_batch(planes)
    src, base = torch.from_numpy(keep.copy()).cuda(), torch.from_numpy(keep_base.copy()).cuda()

    def src_of(i):
        return keep[s_at[i]:s_at[i] + cases[i][1]]

    def base_of(i):
        return np.zeros(cases[i][1], dtype=np.uint8) if b_at[i] is None else keep_base[b_at[i]:b_at[i] + cases[i][1]]

    planar = run(mod, filt, cases, src, s_at, base, b_at, d_total, d_at, False)
    check(mod, cases, planar, d_at, lambda i: split_model(src_of(i) ^ base_of(i), cases[i][0]))
    joined = run(mod, filt, cases, src, s_at, base, b_at, d_total, d_at, True)
    check(mod, cases, joined, d_at, lambda i: join_model(src_of(i), cases[i][0]) ^ base_of(i))
    del joined
    back_cases = [(E, size, do, so) for E, size, so, do in cases]
    _, k_at, _, k_total = mod.place(back_cases)
    back = run(mod, filt, back_cases, planar, d_at, base, b_at, k_total, k_at, True)
    check(mod, back_cases, back, k_at, lambda i: src_of(i))
    assert np.array_equal(src.cpu().numpy(), keep) and np.array_equal(base.cpu().numpy(), keep_base), "the source or a base changed"
    del back, planar
    # a base that is its buffer's src: zeros
    zeros = run(mod, filt, cases, src, s_at, src, s_at, d_total, d_at, False)
    check(mod, cases, zeros, d_at, lambda i: np.zeros(cases[i][1], dtype=np.uint8))


@pytest.mark.parametrize("planes", ["bytes", "bits"])
def test_without_bases_the_result_is_the_plain_entries_byte_for_byte(planes):
    import torch
    L = lib()
    filt, mod, _, _ = FILTERS[planes]
    cases, s_at, d_at, s_total, d_total, b_at, keep, _ = the_batch(planes)
    src = torch.from_numpy(keep.copy()).cuda()
    k = len(cases)
    for join in (False, True):
        got = run(mod, filt, cases, src, s_at, None, b_at, d_total, d_at, join)
        want = torch.full((d_total,), mod.FILL, dtype=torch.uint8, device="cuda")
        fn = getattr(L, "LizardGPU_%s%sPlanes_device" % ("join" if join else "split", "Bit" if filt else ""))
        assert fn(k, (C.c_void_p * k)(*[want.data_ptr() + d for d in d_at]), (C.c_void_p * k)(*[src.data_ptr() + s for s in s_at]),
                  (C.c_size_t * k)(*[c[1] for c in cases]), (C.c_uint32 * k)(*[c[0] for c in cases]),
                  C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert torch.equal(got, want)
        # ... and with an array of null bases
        again = run(mod, filt, cases, src, s_at, src, [None] * k, d_total, d_at, join)
        assert torch.equal(again, want)


def test_every_bad_argument_launches_nothing_and_no_buffers_is_fine():
    import torch
    L = lib()
    n, size = 3, 4096
    src = torch.arange(n * size, dtype=torch.int32, device="cuda").to(torch.uint8)
    base = (torch.arange(n * size, dtype=torch.int32, device="cuda") * 7 + 1).to(torch.uint8)
    dst = torch.full((n * size,), pi.FILL, dtype=torch.uint8, device="cuda")
    srcs, dsts = [src.data_ptr() + i * size for i in range(n)], [dst.data_ptr() + i * size for i in range(n)]
    bases = [base.data_ptr() + i * size for i in range(n)]
    sizes, elems = [size] * n, [2, 4, 8]
    null_at = lambda v, i: v[:i] + [None] + v[i + 1:]
    bad = {
        "no dsts": (srcs, None, sizes, elems, BYTES), "no srcs": (None, dsts, sizes, elems, BITS), "no sizes": (srcs, dsts, None, elems, BYTES),
        "no element sizes": (srcs, dsts, sizes, None, BITS),
        "element size 0": (srcs, dsts, sizes, [2, 0, 8], BYTES), "element size 3": (srcs, dsts, sizes, [2, 4, 3], BITS),
        "element size 16": (srcs, dsts, sizes, [16, 4, 8], BYTES),
        "a null src": (null_at(srcs, 2), dsts, sizes, elems, BYTES), "a null dst": (srcs, null_at(dsts, 1), sizes, elems, BITS),
        "2^32 tiles": (srcs, dsts, [size, size, (1 << 32) * pi.TILE - 2 * pi.TILE], elems, BYTES),
        "filter 2": (srcs, dsts, sizes, elems, 2), "filter 2^32 - 1": (srcs, dsts, sizes, elems, 0xFFFFFFFF),
    }
    for join in (False, True):
        for what, (s, d, z, e, f) in bad.items():
            s0, p0 = stats(), plain_stats()
            if z is None:                                        # (the helper sizes its arrays by `sizes`)
                fn = L.LizardGPU_joinPlanesXor_device if join else L.LizardGPU_splitPlanesXor_device
                rc = fn(n, (C.c_void_p * n)(*d), (C.c_void_p * n)(*s), (C.c_void_p * n)(*bases), None, (C.c_uint32 * n)(*e), f, None)
            else:
                rc = call(join, s, d, bases, z, e, f)
            assert rc == -ERR_ARG, (what, rc)
            assert L.LizardGPU_lastError() != b"", what
            assert stats() == s0 and plain_stats() == p0, what
            torch.cuda.synchronize()
            assert bool((dst == pi.FILL).all()), (what, "dst changed")
        for filt, split_model, join_model in ((BYTES, pi.split_model, pi.join_model), (BITS, bi.bits_split_model, bi.bits_join_model)):
            # no buffers: 0, with or without arrays, nothing touched
            s0, p0 = stats(), plain_stats()
            assert call(join, srcs, dsts, bases, sizes, elems, filt, n=0) == 0 and call(join, None, None, None, [], None, filt, n=0) == 0
            assert stats() == s0 and bool((dst == pi.FILL).all())
            # empty entries are skipped, their pointers may be null; a batch of nothing else launches nothing
            assert call(join, [None, None], [None, None], [None, None], [0, 0], [2, 8], filt) == 0
            assert stats() == s0
            assert call(join, [None, srcs[1]], [None, dsts[1]], [None, bases[1]], [0, size], [4, 4], filt) == 0
            assert [b - a for a, b in zip(s0, stats())] == [0 if join else 2, 2 if join else 0, size, 1]
            assert plain_stats() == p0
            got = dst.cpu().numpy()
            s1, b1 = src.cpu().numpy()[size:2 * size], base.cpu().numpy()[size:2 * size]
            want = join_model(s1, 4) ^ b1 if join else split_model(s1 ^ b1, 4)
            assert (got[:size] == pi.FILL).all() and (got[2 * size:] == pi.FILL).all() and np.array_equal(got[size:2 * size], want)
            dst.fill_(pi.FILL)
