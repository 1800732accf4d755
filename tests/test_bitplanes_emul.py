"""The bodies of lz_bitplanes_split_kernel / lz_bitplanes_join_kernel (lizard_amd/csrc/bitplanes_kernels.h: one tile of a batch of
buffers, its buffer found by bisection of the batch table) on the CPU SIMT emulator, under both lane schedules, against the numpy
model of the bit-plane layout (unpackbits, transpose, packbits; then the copied bytes).  One batch (tests/bitplanes_inputs.py) holds
every element size with every size at which the code takes another path, under pairs of src / dst offsets from a 16-byte boundary
(every pair up to 4 KiB), and 300 one-byte buffers: every dst equals the model, the 64 bytes of 0x5A around every dst are intact, no
tile read outside its buffer's src or wrote outside its dst, and join(split(x)) == x for the same batch."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import bitplanes_inputs as bi

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
SEEDS = (1, 0x9E3779B9)


class Entry(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("size", C.c_uint64), ("elem", C.c_uint32), ("firstTile", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libbitplanes_emul.so from simt.cpp + bitplanes_api.cpp, the way test_planes_emul.py builds its library."""
    out = os.path.join(EMUL, "libbitplanes_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "bitplanes_api.cpp")]
    csrc = os.path.join(util.ROOT, "lizard_amd", "csrc")
    deps = srcs + [os.path.join(EMUL, "lz_wave.h"), os.path.join(csrc, "planes_kernels.h"), os.path.join(csrc, "bitplanes_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_bitplanes.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_uint]
    L.emul_bitplanes.restype = C.c_uint
    L.emul_bitplanes_tile_bytes.restype = C.c_uint
    L.emul_bitplanes_entry_bytes.restype = C.c_uint
    L.emul_bitplanes_step_elems.restype = C.c_uint
    return L


def test_the_entry_the_tile_and_the_step_are_the_ones_the_host_file_and_the_inputs_assume():
    L = lib()
    assert L.emul_bitplanes_entry_bytes() == C.sizeof(Entry) == 32
    assert L.emul_bitplanes_tile_bytes() == bi.TILE == 16384
    assert L.emul_bitplanes_step_elems() == bi.STEP
    assert all(bi.TILE // E % bi.STEP == 0 for E in bi.ELEMS), "a tile is whole wave steps for every element size"


def test_the_numpy_models_invert_each_other_and_follow_the_documented_formula():
    rs = np.random.RandomState(11)
    for E in bi.ELEMS:
        for size in (0, 1, 7, 8 * E - 1, 8 * E, 8 * E + 1, 1003):
            a = rs.randint(0, 256, size, dtype=np.uint8)
            s = bi.bits_split_model(a, E)
            assert s.size == size and np.array_equal(bi.bits_join_model(s, E), a)
        a = rs.randint(0, 256, 19 * E + 1, dtype=np.uint8)      # dst[k * P + j] = sum of bit_k(element 8 j + b) << b, spelled out
        n8, P = 16, 2
        want = a.copy()
        for k in range(8 * E):
            for j in range(P):
                want[k * P + j] = sum(((int(a[(8 * j + b) * E + k // 8]) >> (k % 8)) & 1) << b for b in range(8))
        assert np.array_equal(bi.bits_split_model(a, E), want) and np.array_equal(want[n8 * E:], a[n8 * E:])


def arena(nbytes):
    """A uint8 array of nbytes whose first byte is 16-byte aligned."""
    raw = np.empty(nbytes + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip:skip + nbytes]


def run(L, cases, src, s_at, d_total, d_at, join, seed):
    """The batch through the emulator the way the host file drives the kernel: the non-empty buffers' entries, tiles numbered through.
    Returns the dst arena."""
    dst = arena(d_total)
    dst[:] = bi.FILL
    live = [(c, s, d) for c, s, d in zip(cases, s_at, d_at) if c[1]]
    tab, tiles = (Entry * len(live))(), 0
    for e, ((E, size, _, _), s, d) in zip(tab, live):
        e.src, e.dst, e.size, e.elem, e.firstTile = src.ctypes.data + s, dst.ctypes.data + d, size, E, tiles
        tiles += bi.tiles_of(E, size)
    bad = L.emul_bitplanes(tab, len(live), tiles, 1 if join else 0, seed)
    assert bad == 0, "%d tiles read outside their buffer's src or wrote outside its dst" % bad
    return dst


def check(cases, dst, d_at, want):
    """Every dst is want(i), and every byte of the arena that belongs to no dst still holds the fill."""
    mask = np.ones(dst.size, dtype=bool)
    for i, ((E, size, so, do), d) in enumerate(zip(cases, d_at)):
        got = dst[d:d + size]
        assert np.array_equal(got, want(i)), ("buffer", i, "E", E, "size", size, "offsets", so, do,
                                              "first difference at", int(np.flatnonzero(got != want(i))[0]))
        mask[d:d + size] = False
    assert (dst[mask] == bi.FILL).all(), "a byte outside every dst changed"
    assert all(d >= bi.GUARD for d in d_at) and dst.size - (d_at[-1] + cases[-1][1]) >= bi.GUARD


def test_split_and_join_a_batch_against_the_numpy_model():
    L = lib()
    cases = bi.batch()
    assert {c[0] for c in cases} == set(bi.ELEMS) and {(c[2], c[3]) for c in cases} == {(a, b) for a in bi.OFFSETS for b in bi.OFFSETS}
    assert len(cases) > 1000 and max(bi.tiles_of(c[0], c[1]) for c in cases) == 3
    s_at, d_at, s_total, d_total = bi.place(cases)
    assert s_total + 3 * d_total < 12 << 20
    src = arena(s_total)
    src[:] = bi.source(s_total)
    assert all((src.ctypes.data + s) % 16 == c[2] for c, s in zip(cases, s_at))
    keep = src.copy()
    models = [bi.bits_split_model(keep[s:s + c[1]], c[0]) for c, s in zip(cases, s_at)]
    for seed in SEEDS:
        planar = run(L, cases, src, s_at, d_total, d_at, False, seed)
        assert all((planar.ctypes.data + d) % 16 == c[3] for c, d in zip(cases, d_at))
        check(cases, planar, d_at, lambda i: models[i])
        assert np.array_equal(src, keep), "the source changed"
        # join against its own model on the same bytes ...
        joined = run(L, cases, src, s_at, d_total, d_at, True, seed)
        check(cases, joined, d_at, lambda i: bi.bits_join_model(keep[s_at[i]:s_at[i] + cases[i][1]], cases[i][0]))
        # ... and join(split(x)) == x: the planar buffers are the sources now, at the dst offsets, into dsts at the src offsets
        back_cases = [(E, size, do, so) for E, size, so, do in cases]
        _, b_at, _, b_total = bi.place(back_cases)
        back = run(L, back_cases, planar, d_at, b_total, b_at, True, seed)
        check(back_cases, back, b_at, lambda i: keep[s_at[i]:s_at[i] + cases[i][1]])
