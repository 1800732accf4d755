"""CPU: the sweep of the 24-bit LDS table of levels 10 / 30 (lizard_amd/csrc/lz_block.h) on the SIMT emulator.  The one-slot sweep
(lz_tab_sweep_narrow) and the four-slot one (lz_tab_sweep_wide, lz_tab_fresh_wide) run on copies of one random table image
(tests/emul/sweep_api.cpp) and must leave the same bytes, which are also those of a model written here from the table's definition:
a slot whose 17-bit position is 65 536 or more behind Ps becomes (Ps + 65 536) mod 2^17 with check bits 0, every other slot and the
trash slot (index 4 096) stay.  Then the sweep_* inputs of tests/producer_tail_inputs.py through the emulated producer / consumer
kernel at levels 10 and 30 against the oracle."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import producer_tail_inputs as inputs
from test_producer_round_emul import emul_split

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
SLOTS = 4096
HI_AT = 2 * SLOTS + 4                    # lz_tab_bind: `hi` starts 4 bytes behind the trash slot's u16
TAB_BYTES = 3 * SLOTS + 8                # LZ_TAB_BYTES(12)
POSITIONS = (1, 32768, 32769, 65536, 65537, 131071, 131072, 200000)
AGES = (65535, 65536, 65537, 131071)


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libsweep_emul.so from simt.cpp + sweep_api.cpp, the way test_planes_emul.py builds its library."""
    out = os.path.join(EMUL, "libsweep_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "sweep_api.cpp")]
    csrc = os.path.join(util.ROOT, "lizard_amd", "csrc")
    deps = srcs + [os.path.join(EMUL, "lz_wave.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_sweep_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_uint]
    L.emul_sweep_pair.restype = None
    L.emul_sweep_table_bytes.restype = C.c_uint
    L.emul_sweep_default_is_wide.restype = C.c_int
    return L


def image_at(image, skew):
    """A copy of the table image whose first byte lies `skew` bytes (0 or 4) behind a multiple of 8: a workgroup's tables are
    LZ_TAB_BYTES + 4 apart, so every other producer's table is dword-aligned only."""
    raw = np.empty(TAB_BYTES + 16, dtype=np.uint8)
    at = (-raw.ctypes.data) % 8 + skew
    view = raw[at:at + TAB_BYTES]
    view[:] = image
    assert view.ctypes.data % 8 == skew
    return view


def entries(image):
    lo = image[:2 * (SLOTS + 1)].view("<u2").astype(np.uint32)
    hi = image[HI_AT:HI_AT + SLOTS + 1].astype(np.uint32)
    return lo | hi << 16


def random_image(rng, Ps):
    """4 097 random 24-bit slots and random bytes in the gaps; slots 0.., 1 000.., 2 045.. and 4 092.. are aged exactly AGES (with
    check bits all 0, all 1 and random), so that every one of a step's four slots and both ends of the table meet every age."""
    image = rng.integers(0, 256, TAB_BYTES, dtype=np.uint8)
    lo = image[:2 * (SLOTS + 1)].view("<u2")
    hi = image[HI_AT:HI_AT + SLOTS + 1]
    for base, check in ((0, 0), (1000, 127), (2045, None), (SLOTS - len(AGES), None)):
        for shift in range(4 if base in (0, 1000) else 1):
            for k, age in enumerate(AGES):
                slot = base + 4 * shift + (k + shift) % 4
                ent = (Ps - age) & 0x1FFFF | (int(rng.integers(0, 128)) if check is None else check) << 17
                lo[slot], hi[slot] = ent & 0xFFFF, ent >> 16
    return image


def model(image, Ps, fresh):
    want = image.copy()
    ent = entries(image)[:SLOTS]
    deadslot = np.ones(SLOTS, bool) if fresh else ((Ps - ent) & 0x1FFFF) >= 65536
    dead = (Ps + 65536) & 0x1FFFF
    want[:2 * SLOTS].view("<u2")[deadslot] = dead & 0xFFFF
    want[HI_AT:HI_AT + SLOTS][deadslot] = dead >> 16
    return want


def test_the_library_is_the_layout_the_model_assumes():
    assert lib().emul_sweep_table_bytes() == TAB_BYTES
    assert lib().emul_sweep_default_is_wide() == 1


@pytest.mark.parametrize("Ps", POSITIONS)
def test_wide_sweep_leaves_what_the_narrow_sweep_leaves(Ps):
    rng = np.random.default_rng(Ps)
    for skew in (0, 4):
        image = random_image(rng, Ps)
        ages = (Ps - entries(image)[:SLOTS]) & 0x1FFFF
        assert all((ages == a).sum() >= 10 for a in AGES) and 0.3 < (ages >= 65536).mean() < 0.7
        narrow, wide = image_at(image, skew), image_at(image, skew)
        lib().emul_sweep_pair(narrow.ctypes.data, wide.ctypes.data, Ps, 0, Ps + skew)
        want = model(image, Ps, False)
        assert np.array_equal(narrow, want), (Ps, skew, np.flatnonzero(narrow != want)[:8])
        assert np.array_equal(wide, want), (Ps, skew, np.flatnonzero(wide != want)[:8])
        # the trash slot and the bytes around it came back as they were
        for a, b in ((2 * SLOTS, HI_AT), (HI_AT + SLOTS, TAB_BYTES)):
            assert np.array_equal(wide[a:b], image[a:b]), (Ps, skew, a)


def test_fresh_is_a_sweep_with_fresh_set():
    rng = np.random.default_rng(7)
    for skew in (0, 4):
        image = random_image(rng, 1)
        narrow, wide = image_at(image, skew), image_at(image, skew)
        lib().emul_sweep_pair(narrow.ctypes.data, wide.ctypes.data, 0, 1, 11 + skew)
        want = model(image, 0, True)
        assert (entries(want)[:SLOTS] == 0x10000).all()
        assert np.array_equal(narrow, want) and np.array_equal(wide, want), skew


@functools.lru_cache(maxsize=None)
def sweep_blocks():
    return tuple((name, data) for name, data in inputs.all_blocks() if name.startswith("sweep_"))


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_sweep_inputs_through_the_split_kernel(level):
    """The blocks whose decisions hang on a sweep (a word 65 535 back found, the same word 65 536 back not; entries 2^17 + 100 old
    with the same bytes and check bits) through the emulated kernel, whose producer calls lz_tab_sweep()."""
    want = inputs.expected(level)
    assert len(sweep_blocks()) == 7
    for case, (name, data) in enumerate(sweep_blocks()):
        assert emul_split(data, len(data), level, nprod=1, ncons=1, seed=100 + case) == [want[name]], (level, name)
