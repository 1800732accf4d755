"""The bodies of lz_planes_split_kernel / lz_planes_join_kernel (lizard_amd/csrc/planes_kernels.h: one tile of a batch of buffers, its
buffer found by bisection of the batch table) on the CPU SIMT emulator, under both lane schedules, against a numpy model of the
layout (a[:n*E].reshape(n, E).T, then the tail).  One batch (tests/planes_inputs.py) holds every element size with every size at
which the code takes another path, under pairs of src / dst offsets from a 16-byte boundary (every pair up to 4 KiB), and 300 one-byte buffers: every
dst equals the model, the 64 bytes of 0x5A around every dst are intact, no tile read outside its buffer's src or wrote outside its
dst, and join(split(x)) == x for the same batch."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import planes_inputs as pi

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
SEEDS = (1, 0x9E3779B9)


class Entry(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("size", C.c_uint64), ("elem", C.c_uint32), ("firstTile", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libplanes_emul.so from simt.cpp + planes_api.cpp, the way test_unframes_emul.py builds its library."""
    out = os.path.join(EMUL, "libplanes_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "planes_api.cpp")]
    deps = srcs + [os.path.join(EMUL, "lz_wave.h"), os.path.join(util.ROOT, "lizard_amd", "csrc", "planes_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_planes.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_uint]
    L.emul_planes.restype = C.c_uint
    L.emul_planes_tile_bytes.restype = C.c_uint
    L.emul_planes_entry_bytes.restype = C.c_uint
    return L


def test_the_entry_and_the_tile_are_the_ones_the_host_file_and_the_inputs_assume():
    L = lib()
    assert L.emul_planes_entry_bytes() == C.sizeof(Entry) == 32
    assert L.emul_planes_tile_bytes() == pi.TILE
    assert pi.TILE % (64 * 16 * 8) == 0


def arena(nbytes):
    """A uint8 array of nbytes whose first byte is 16-byte aligned."""
    raw = np.empty(nbytes + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip:skip + nbytes]


def run(L, cases, src, s_at, d_total, d_at, join, seed):
    """The batch through the emulator the way the host file drives the kernel: the non-empty buffers' entries, tiles numbered through.
    Returns the dst arena."""
    dst = arena(d_total)
    dst[:] = pi.FILL
    live = [(c, s, d) for c, s, d in zip(cases, s_at, d_at) if c[1]]
    tab, tiles = (Entry * len(live))(), 0
    for e, ((E, size, _, _), s, d) in zip(tab, live):
        e.src, e.dst, e.size, e.elem, e.firstTile = src.ctypes.data + s, dst.ctypes.data + d, size, E, tiles
        tiles += pi.tiles_of(E, size)
    bad = L.emul_planes(tab, len(live), tiles, 1 if join else 0, seed)
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
    assert (dst[mask] == pi.FILL).all(), "a byte outside every dst changed"
    assert all(d >= pi.GUARD for d in d_at) and dst.size - (d_at[-1] + cases[-1][1]) >= pi.GUARD


def test_split_and_join_a_batch_against_the_numpy_model():
    L = lib()
    cases = pi.batch()
    assert {c[0] for c in cases} == set(pi.ELEMS) and {(c[2], c[3]) for c in cases} == {(a, b) for a in pi.OFFSETS for b in pi.OFFSETS}
    assert len(cases) > 1000 and max(pi.tiles_of(c[0], c[1]) for c in cases) == 3
    s_at, d_at, s_total, d_total = pi.place(cases)
    src = arena(s_total)
    src[:] = pi.source(s_total)
    assert all((src.ctypes.data + s) % 16 == c[2] for c, s in zip(cases, s_at))
    keep = src.copy()
    for seed in SEEDS:
        planar = run(L, cases, src, s_at, d_total, d_at, False, seed)
        assert all((planar.ctypes.data + d) % 16 == c[3] for c, d in zip(cases, d_at))
        check(cases, planar, d_at, lambda i: pi.split_model(keep[s_at[i]:s_at[i] + cases[i][1]], cases[i][0]))
        assert np.array_equal(src, keep), "the source changed"
        # join against its own model on the same bytes ...
        joined = run(L, cases, src, s_at, d_total, d_at, True, seed)
        check(cases, joined, d_at, lambda i: pi.join_model(keep[s_at[i]:s_at[i] + cases[i][1]], cases[i][0]))
        # ... and join(split(x)) == x: the planar buffers are the sources now, at the dst offsets, into dsts at the src offsets
        back_cases = [(E, size, do, so) for E, size, so, do in cases]
        _, b_at, _, b_total = pi.place(back_cases)
        back = run(L, back_cases, planar, d_at, b_total, b_at, True, seed)
        check(back_cases, back, b_at, lambda i: keep[s_at[i]:s_at[i] + cases[i][1]])
