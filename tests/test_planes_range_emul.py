"""The body of lz_planes_range_kernel (lizard_amd/csrc/planes_range_kernels.h: one tile of a batch of element ranges joined out of
pieces of their planes, its item found by bisection of the batch table) on the CPU SIMT emulator, under both lane schedules, against
numpy: join(split)[first * E : last * E], optionally XOR the base's slice, with the join models of tests/planes_inputs.py and
tests/bitplanes_inputs.py.  The pieces are the byte ranges of LizardGPU_planesRangeBytes (lizard_slice_host.c, compiled alone:
tests/test_planes_range.py checks it against the layouts) cut out of the split bytes and laid down ONE BY ONE, each at its own offset
from a 16-byte boundary with 64 bytes of 0x5A around it, so a read one byte outside a piece reads no neighbouring plane byte and is
counted.  One batch holds every element size with both filters, pieces at every offset 0 - 15, first % 128 in {0, 1, 8, 127} for bit
planes and first % 16 in {0, 1, 15} for byte planes, `last` inside and equal to the ragged end, ranges of more than one tile, empty
items and 50 one-element items.  Every dst equals the model, the 64 guard bytes around every dst and every piece are intact, and no
access fell outside the item's pieces, base and dst (tests/emul/planes_range_api.cpp tests every access)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import planes_inputs as pi
import bitplanes_inputs as bi
import test_planes_range as pr

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
SEEDS = (1, 0x9E3779B9)
BYTES, BITS = 0, 1
GUARD, FILL, TILE = 64, 0x5A, pi.TILE


class Entry(C.Structure):
    _fields_ = [("dst", C.c_uint64), ("base", C.c_uint64), ("nElems", C.c_uint64), ("first", C.c_uint64), ("last", C.c_uint64),
                ("elem", C.c_uint32), ("filter", C.c_uint32), ("firstTile", C.c_uint32), ("firstPiece", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libplanes_range_emul.so from simt.cpp + planes_range_api.cpp, the way test_planes_emul.py builds its library."""
    out = os.path.join(EMUL, "libplanes_range_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "planes_range_api.cpp")]
    deps = srcs + [os.path.join(EMUL, "lz_wave.h")] + [os.path.join(util.ROOT, "lizard_amd", "csrc", h)
                                                      for h in ("planes_kernels.h", "bitplanes_kernels.h", "planes_range_kernels.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_planes_range.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_uint]
    L.emul_planes_range.restype = C.c_uint
    L.emul_planes_range_tile_bytes.restype = C.c_uint
    L.emul_planes_range_entry_bytes.restype = C.c_uint
    return L


def test_the_entry_and_the_tile_are_the_ones_the_host_file_and_the_inputs_assume():
    L = lib()
    assert L.emul_planes_range_entry_bytes() == C.sizeof(Entry) == 56
    assert L.emul_planes_range_tile_bytes() == TILE


def tiles_of(E, filt, first, last):
    """As lizard_slice_device.c counts them: tiles of the range's elements, for bit planes from the group of 8 that holds `first`."""
    start = first - first % 8 if filt == BITS else first
    return (((last - start) * E + TILE - 1) // TILE) if last > first else 0


def items():
    """[(E, filter, n, first, last)]"""
    out = []
    for E in (1, 2, 4, 8):
        # bit planes: two tiles and a ragged end of whole quads, groups of 8, raw elements
        n = TILE // E + 3 * 128 + 5 * 8 + 3
        n8 = n - n % 8
        firsts = (0, 1, 8, 127, 256, 257, 264, 383)
        assert {f % 128 for f in firsts} == {0, 1, 8, 127}
        for f in firsts:
            for last in (n, n8, n8 - 1, n - 1, f + 1, f + 130, f + 128 + 128, n - 200, TILE // E + f):
                out.append((E, BITS, n, f, last))
        out.append((E, BITS, n, n8, n))                            # the raw elements alone
        out.append((E, BITS, n, n8 + 1, n - 1))
        out.append((E, BITS, n, n8 - 3, n8 + 2))                   # the last group and raw elements
        for small in (1, 7, 8, 9, 127, 128, 129, 300):
            for f, last in ((0, small), (small // 2, small), (0, small - small % 8), (min(1, small), small), (small // 3, 2 * small // 3 + 1)):
                out.append((E, BITS, small, f, last))
        # byte planes: two tiles and a ragged end
        n = TILE // E + 1024 + 16 * 3 + 5
        firsts = (0, 1, 15, 16, 17, 31, 1025)
        assert {f % 16 for f in firsts} == {0, 1, 15}
        for f in firsts:
            for last in (n, n - 5, f + 1, f + 15, f + 16, f + 17, f + 1024, f + 1030, TILE // E + f + 3):
                out.append((E, BYTES, n, f, last))
        for small in (1, 15, 16, 17, 100):
            for f, last in ((0, small), (small // 2, small), (min(1, small), small)):
                out.append((E, BYTES, small, f, last))
        out += [(E, BITS, 1000, 500, 500), (E, BYTES, 1000, 0, 0), (E, BITS, 0, 0, 0), (E, BYTES, 0, 0, 0), (E, BITS, 1000, 1000, 1000)]   # empty items
    for i in range(50):                                            # one-element items
        E = (1, 2, 4, 8)[i % 4]
        out.append((E, (BITS, BYTES)[(i // 4) % 2], 150, 3 * i, 3 * i + 1))
    return out


def arena(nbytes):
    """A uint8 array of nbytes whose first byte is 16-byte aligned."""
    raw = np.empty(nbytes + 16, dtype=np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip:skip + nbytes]


@functools.lru_cache(maxsize=None)
def batch():
    """The whole batch laid out once: (cases, per item (its pieces as (position, bytes), base, base position, dst position, expected
    bytes), bytes of the piece arena, of the base arena, of the dst arena)."""
    rng = np.random.RandomState(11)
    cases, plan, pos_p, pos_b, pos_d = items(), [], 0, 0, GUARD
    for idx, (E, filt, n, first, last) in enumerate(cases):
        src = rng.randint(0, 256, n * E, dtype=np.uint8)
        split = bi.bits_split_model(src, E) if filt == BITS else pi.split_model(src, E)
        joined = (bi.bits_join_model(split, E) if filt == BITS else pi.join_model(split, E))[first * E:last * E]
        assert np.array_equal(joined, src[first * E:last * E])
        base = rng.randint(0, 256, (last - first) * E, dtype=np.uint8) if idx % 2 else None
        want = joined if base is None else joined ^ base
        ranges = pr.ranges_of(n, E, filt, first, last)
        assert len(ranges) == (8 * E + 1 if filt == BITS else E)
        off = idx % 16
        pieces = []
        for q, (lo, hi) in enumerate(ranges):
            pos_p += GUARD
            pos_p += (-(pos_p) + off + 3 * q) % 16                 # the piece's offset from a 16-byte boundary: every value 0 - 15 occurs
            pieces.append((pos_p, split[lo:hi]))
            pos_p += hi - lo
        b_at = None
        if base is not None:
            pos_b += (-(pos_b) + (off + 5) % 16) % 16
            b_at = pos_b
            pos_b += base.size + 1
        pos_d += (-(pos_d) + (7 * idx + 3) % 16) % 16
        d_at = pos_d
        pos_d += (last - first) * E + GUARD
        plan.append((pieces, base, b_at, d_at, want))
    return cases, plan, pos_p + GUARD + 16, pos_b + 16, pos_d + 16


def run(L, seed):
    cases, plan, p_total, b_total, d_total = batch()
    parena, barena, darena = arena(p_total), arena(b_total), arena(d_total)
    parena[:] = FILL
    barena[:] = 0
    darena[:] = FILL
    for pieces, base, b_at, d_at, want in plan:
        for at, data in pieces:
            parena[at:at + data.size] = data
        if base is not None:
            barena[b_at:b_at + base.size] = base
    keep = parena.copy()
    live = [(c, p) for c, p in zip(cases, plan) if c[4] > c[3]]
    tab, tiles, addrs, allow_at, allow = (Entry * len(live))(), 0, [], [0], []
    for e, ((E, filt, n, first, last), (pieces, base, b_at, d_at, want)) in zip(tab, live):
        e.dst, e.base = darena.ctypes.data + d_at, 0 if base is None else barena.ctypes.data + b_at
        e.nElems, e.first, e.last, e.elem, e.filter, e.firstTile, e.firstPiece = n, first, last, E, filt, tiles, len(addrs)
        tiles += tiles_of(E, filt, first, last)
        for at, data in pieces:
            addrs.append(parena.ctypes.data + at)
            allow += [parena.ctypes.data + at, parena.ctypes.data + at + data.size]
        if base is not None:
            allow += [barena.ctypes.data + b_at, barena.ctypes.data + b_at + base.size]
        allow_at.append(len(allow) // 2)
    offsets = {(parena.ctypes.data + at) % 16 for pieces, *_ in plan for at, data in pieces if data.size}
    assert offsets == set(range(16)), offsets
    assert max(tiles_of(*c[:2], *c[3:]) for c in cases) >= 2 and len(live) > 64
    bad = L.emul_planes_range(tab, len(live), (C.c_uint64 * len(addrs))(*addrs), tiles, (C.c_uint64 * len(allow_at))(*allow_at),
                              (C.c_uint64 * len(allow))(*allow), seed)
    assert bad == 0, "%d accesses outside the item's pieces, base and dst" % bad
    assert np.array_equal(parena, keep), "a piece or a guard byte around one changed"
    mask = np.ones(darena.size, dtype=bool)
    for i, ((E, filt, n, first, last), (pieces, base, b_at, d_at, want)) in enumerate(zip(cases, plan)):
        got = darena[d_at:d_at + want.size]
        assert np.array_equal(got, want), ("item", i, "E", E, "filter", filt, "n", n, "range", first, last, "xor", base is not None,
                                           "first difference at byte", int(np.flatnonzero(got != want)[0]))
        mask[d_at:d_at + want.size] = False
    assert (darena[mask] == FILL).all(), "a byte outside every dst changed"


def test_a_batch_of_ranges_against_the_numpy_model_under_both_lane_schedules():
    L = lib()
    for seed in SEEDS:
        run(L, seed)
