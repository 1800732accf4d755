"""The bodies of the XOR-with-base kernels (lz_planes_xor_tile of lizard_amd/csrc/planes_kernels.h, lz_bitplanes_xor_tile of
bitplanes_kernels.h: split writes split(src ^ base), join writes join(src) ^ base) on the CPU SIMT emulator, under both lane
schedules, against the numpy models of tests/planes_inputs.py / tests/bitplanes_inputs.py applied to src ^ base.  For both filters
and both directions the batch is the one the plain kernels' tests move — every element size with every size at which the code takes
another path, pairs of src / dst offsets from a 16-byte boundary, 300 one-byte buffers, up to three tiles per buffer —, each buffer's
base sits at its own offset from a 16-byte boundary (every value of OFFSETS, not always the src's) and about every fifth entry has
no base (base == 0: the plain path, the plain model).  Every dst equals the model, the 0x5A guards are intact, src and base are
unchanged, every single access of a tile lies inside its buffer's src[0..size) or base[0..size) (reads) or dst[0..size) (writes),
join(split(x, b), b) == x, and base == src gives zeros."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import planes_inputs as pi
import bitplanes_inputs as bi
from planes_xor_inputs import base_offsets, place_bases

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
SEEDS = (1, 0x9E3779B9)


class Entry(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("base", C.c_uint64), ("size", C.c_uint64), ("elem", C.c_uint32),
                ("firstTile", C.c_uint32)]


# filter name -> (inputs module, split model, join model)
FILTERS = {"bytes": (pi, pi.split_model, pi.join_model), "bits": (bi, bi.bits_split_model, bi.bits_join_model)}


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libplanes_xor_emul.so from simt.cpp + planes_xor_api.cpp, the way test_planes_emul.py builds its library."""
    out = os.path.join(EMUL, "libplanes_xor_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "planes_xor_api.cpp")]
    csrc = os.path.join(util.ROOT, "lizard_amd", "csrc")
    deps = srcs + [os.path.join(EMUL, "lz_wave.h"), os.path.join(csrc, "planes_kernels.h"), os.path.join(csrc, "bitplanes_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_planes_xor.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    L.emul_planes_xor.restype = C.c_uint
    for name in ("emul_planes_xor_tile_bytes", "emul_planes_xor_entry_bytes", "emul_planes_entry_bytes"):
        getattr(L, name).restype = C.c_uint
    return L


def test_the_entry_is_40_bytes_on_both_sides_and_the_plain_entry_keeps_its_32():
    L = lib()
    assert L.emul_planes_xor_entry_bytes() == C.sizeof(Entry) == 40
    assert (Entry.src.offset, Entry.dst.offset, Entry.base.offset, Entry.size.offset, Entry.elem.offset, Entry.firstTile.offset) == (0, 8, 16, 24, 32, 36)
    assert L.emul_planes_entry_bytes() == 32
    assert L.emul_planes_xor_tile_bytes() == pi.TILE == bi.TILE


def arena(nbytes):
    """A uint8 array of nbytes whose first byte is 16-byte aligned."""
    raw = np.empty(nbytes + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip:skip + nbytes]


def run(L, mod, cases, src, s_at, base, b_at, d_total, d_at, join, bits, seed):
    """The batch through the emulator the way the host file drives the kernel: the non-empty buffers' entries, tiles numbered through.
    `base`: an arena and b_at the places in it (None: no base).  Returns the dst arena."""
    dst = arena(d_total)
    dst[:] = mod.FILL
    live = [(c, s, b, d) for c, s, b, d in zip(cases, s_at, b_at, d_at) if c[1]]
    tab, tiles = (Entry * len(live))(), 0
    for e, ((E, size, _, _), s, b, d) in zip(tab, live):
        e.src, e.dst, e.size, e.elem, e.firstTile = src.ctypes.data + s, dst.ctypes.data + d, size, E, tiles
        e.base = 0 if b is None else base.ctypes.data + b
        tiles += mod.tiles_of(E, size)
    reads = C.c_ulonglong(0)
    bad = L.emul_planes_xor(tab, len(live), tiles, 1 if join else 0, 1 if bits else 0, seed, C.byref(reads))
    assert bad == 0, "%d tiles read outside their buffer's src and base or wrote outside its dst" % bad
    assert (reads.value > 0) == any(b is not None for _, _, b, _ in live)
    return dst


def check(mod, cases, dst, d_at, want):
    """Every dst is want(i), and every byte of the arena that belongs to no dst still holds the fill."""
    mask = np.ones(dst.size, dtype=bool)
    for i, ((E, size, so, do), d) in enumerate(zip(cases, d_at)):
        got, w = dst[d:d + size], want(i)
        assert np.array_equal(got, w), ("buffer", i, "E", E, "size", size, "offsets", so, do,
                                        "first difference at", int(np.flatnonzero(got != w)[0]))
        mask[d:d + size] = False
    assert (dst[mask] == mod.FILL).all(), "a byte outside every dst changed"
    assert all(d >= mod.GUARD for d in d_at) and dst.size - (d_at[-1] + cases[-1][1]) >= mod.GUARD


@pytest.mark.parametrize("planes", ["bytes", "bits"])
def test_split_and_join_a_batch_with_bases_against_the_numpy_model(planes):
    L = lib()
    mod, split_model, join_model = FILTERS[planes]
    bits = planes == "bits"
    cases = mod.batch()
    assert {c[0] for c in cases} == set(mod.ELEMS) and {(c[2], c[3]) for c in cases} == {(a, b) for a in mod.OFFSETS for b in mod.OFFSETS}
    assert len(cases) > 1000 and max(mod.tiles_of(c[0], c[1]) for c in cases) == 3
    s_at, d_at, s_total, d_total = mod.place(cases)
    b_off = base_offsets(cases, list(mod.OFFSETS))
    b_at, b_total = place_bases(cases, b_off)
    src, base = arena(s_total), arena(b_total)
    src[:] = mod.source(s_total)
    base[:] = mod.source(b_total, seed=6)
    assert all((src.ctypes.data + s) % 16 == c[2] for c, s in zip(cases, s_at))
    assert all((base.ctypes.data + b) % 16 == o for b, o in zip(b_at, b_off) if b is not None)
    with_base = [c for c, o in zip(cases, b_off) if o is not None and c[1]]
    assert {o for o in b_off if o is not None} == set(mod.OFFSETS)
    assert 0.15 < 1 - len(with_base) / sum(1 for c in cases if c[1]) < 0.25
    assert any(o != c[2] for c, o in zip(cases, b_off) if o is not None) and any(o == c[2] for c, o in zip(cases, b_off) if o is not None)
    for E in mod.ELEMS:                                          # with and without a base: every size of every element size
        assert {c[1] for c, o in zip(cases, b_off) if c[0] == E and o is not None} >= set(mod.sizes_for(E)) - {0}
        assert {c[1] for c, o in zip(cases, b_off) if c[0] == E and o is None} >= set(mod.sizes_for(E)) - {0}
    keep, keep_base = src.copy(), base.copy()

    def src_of(i):
        return keep[s_at[i]:s_at[i] + cases[i][1]]

    def base_of(i):
        return np.zeros(cases[i][1], dtype=np.uint8) if b_at[i] is None else keep_base[b_at[i]:b_at[i] + cases[i][1]]

    split_want = [split_model(src_of(i) ^ base_of(i), c[0]) for i, c in enumerate(cases)]
    join_want = [join_model(src_of(i), c[0]) ^ base_of(i) for i, c in enumerate(cases)]
    back_cases = [(E, size, do, so) for E, size, so, do in cases]
    _, k_at, _, k_total = mod.place(back_cases)
    for seed in SEEDS:
        planar = run(L, mod, cases, src, s_at, base, b_at, d_total, d_at, False, bits, seed)
        assert all((planar.ctypes.data + d) % 16 == c[3] for c, d in zip(cases, d_at))
        check(mod, cases, planar, d_at, lambda i: split_want[i])
        # join against its own model on the same bytes ...
        joined = run(L, mod, cases, src, s_at, base, b_at, d_total, d_at, True, bits, seed)
        check(mod, cases, joined, d_at, lambda i: join_want[i])
        # ... and join(split(x, b), b) == x: the planar buffers are the sources now, at the dst offsets, into dsts at the src offsets
        back = run(L, mod, back_cases, planar, d_at, base, b_at, k_total, k_at, True, bits, seed)
        check(mod, back_cases, back, k_at, lambda i: src_of(i))
        assert np.array_equal(src, keep) and np.array_equal(base, keep_base), "the source or a base changed"
    # a base that is its buffer's src: the split is all zeros
    zeros = run(L, mod, cases, src, s_at, src, s_at, d_total, d_at, False, bits, SEEDS[0])
    check(mod, cases, zeros, d_at, lambda i: np.zeros(cases[i][1], dtype=np.uint8))
    assert np.array_equal(src, keep)


@pytest.mark.parametrize("planes", ["bytes", "bits"])
def test_a_batch_without_any_base_is_the_plain_filter(planes):
    L = lib()
    mod, split_model, join_model = FILTERS[planes]
    cases = [c for c in mod.batch() if c[1] > 1][::7]
    s_at, d_at, s_total, d_total = mod.place(cases)
    src = arena(s_total)
    src[:] = mod.source(s_total)
    none = [None] * len(cases)
    for join, model in ((False, split_model), (True, join_model)):
        got = run(L, mod, cases, src, s_at, None, none, d_total, d_at, join, planes == "bits", SEEDS[1])
        check(mod, cases, got, d_at, lambda i: model(src[s_at[i]:s_at[i] + cases[i][1]], cases[i][0]))
