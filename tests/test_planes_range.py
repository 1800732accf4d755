"""CPU: the arithmetic of a row range (lizard_amd/csrc/lizard_slice_host.c, compiled ALONE; include/lizard_amd.h Part 3d).
LizardGPU_planesRangeBytes against a brute-force model: the index map of the numpy split (tests/planes_inputs.py /
tests/bitplanes_inputs.py) says which split bytes every element has a byte or a bit in; the ranges must cover exactly the set that
elements [first, last) depend on — nothing more for byte planes, less than one byte per bit plane more (so: nothing more) for bit
planes — and ascend.  LizardGPU_frameRangesBound against the obvious sum.  The same calls as a stand-alone program under
AddressSanitizer + UBSan (tests/planes_range_asan_main.c), run directly."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import planes_inputs as pi
import bitplanes_inputs as bi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(util.ROOT, "lizard_amd", "csrc")
_dir = tempfile.mkdtemp(prefix="planes_range_")
BYTES, BITS = 0, 1
SIZES = (0, 1, 7, 8, 9, 127, 128, 129, 1000, 2055)


class Range(C.Structure):
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_uint64)]


@functools.lru_cache(maxsize=None)
def lib():
    out = os.path.join(_dir, "libslice_host.so")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared",
                           os.path.join(CSRC, "lizard_slice_host.c"), "-o", out])
    L = C.CDLL(out)
    L.LizardGPU_planesRangeBytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t]
    L.LizardGPU_planesRangeBytes.restype = C.c_size_t
    L.LizardGPU_frameRangesBound.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    L.LizardGPU_frameRangesBound.restype = C.c_size_t
    return L


def ranges_of(n, E, filt, first, last, room=65):
    out = (Range * 66)()
    out[room].lo = 0xABCDEF
    got = lib().LizardGPU_planesRangeBytes(n, E, filt, first, last, out, room)
    assert out[room].lo == 0xABCDEF
    return [(r.lo, r.hi) for r in out[:got]]


@functools.lru_cache(maxsize=None)
def depends(n, E, filt):
    """(lowest, highest + 1) split byte per PIECE that element i has a bit in, as arrays [pieces][n] — from the split model applied to
    an index map: bit b of split byte x comes from the interleaved byte the model moved there."""
    size = n * E
    pieces = E if filt == BYTES else 8 * E + 1
    lo, hi = np.full((pieces, n), size + 1, dtype=np.int64), np.zeros((pieces, n), dtype=np.int64)
    if filt == BYTES:
        # split_model moves whole bytes: split an array of element numbers
        elem = np.repeat(np.arange(n, dtype=np.int64), E)
        where = pi.split_model(elem, E)                            # where[x] = the element whose byte lies at split byte x
        for x, i in enumerate(where):
            p = x // n if n else 0
            lo[p, i], hi[p, i] = min(lo[p, i], x), max(hi[p, i], x + 1)
        return lo, hi
    n8 = n - n % 8
    P = n8 // 8
    # one-hot per element would be n splits; instead split the bits of the element NUMBER, plane by plane of the number's bits
    owner = np.zeros((size, 8), dtype=np.int64)                    # owner[x, b] = element whose bit lies in bit b of split byte x
    nbits = max(1, int(n).bit_length())
    for t in range(nbits):
        src = np.zeros(size, dtype=np.uint8)
        for i in range(n):
            if (i >> t) & 1:
                src[i * E:(i + 1) * E] = 0xFF
        got = bi.bits_split_model(src, E)
        owner |= (np.unpackbits(got.reshape(-1, 1), axis=1, bitorder="little").astype(np.int64) << t)
    for x in range(size):
        p = x // P if x < 8 * E * P else 8 * E
        for i in set(owner[x].tolist()):
            lo[p, i], hi[p, i] = min(lo[p, i], x), max(hi[p, i], x + 1)
    return lo, hi


def needed(n, E, filt, first, last):
    """The exact set of split bytes elements [first, last) depend on, per piece: sorted arrays."""
    lo, hi = depends(n, E, filt)
    out = []
    for p in range(lo.shape[0]):
        s = set()
        for i in range(first, last):
            s.update(range(int(lo[p, i]), int(hi[p, i])))
        out.append(sorted(s))
    return out


def pairs_for(n):
    if n <= 129:
        return [(a, b) for a in range(n + 1) for b in range(a, n + 1)]
    rng = np.random.RandomState(n)
    out = [(0, n), (0, 0), (n, n), (n - 1, n), (n - n % 8, n)]
    while len(out) < 200:
        a, b = sorted(int(v) for v in rng.randint(0, n + 1, 2))
        out.append((a, b))
    return out


def check_case(n, E, filt):
    """Per piece, the hull [lowest, highest + 1) of the bytes the elements of the range depend on (an element that does not touch a
    piece has the sentinels size + 1 and 0 there): the range must cover it, and exceed it by less than one byte — by nothing."""
    lo, hi = depends(n, E, filt)
    pieces = lo.shape[0]
    for first, last in pairs_for(n):
        got = np.array(ranges_of(n, E, filt, first, last), dtype=np.int64).reshape(-1, 2)
        what = (n, E, filt, first, last, got.tolist())
        assert len(got) == pieces, what
        assert (np.diff(got.reshape(-1)) >= 0).all(), ("not ascending", what)
        if last > first:
            want_lo, want_hi = lo[:, first:last].min(axis=1), hi[:, first:last].max(axis=1)
        else:
            want_lo, want_hi = np.full(pieces, n * E + 1, dtype=np.int64), np.zeros(pieces, dtype=np.int64)
        touched = want_hi > 0
        assert (got[~touched, 0] == got[~touched, 1]).all(), ("a piece no element of the range touches is not empty", what)
        assert (got[touched, 0] <= want_lo[touched]).all() and (got[touched, 1] >= want_hi[touched]).all(), ("does not cover", what)
        excess = (got[touched, 1] - got[touched, 0]) - (want_hi[touched] - want_lo[touched])
        assert (excess < 1).all(), ("exceeds what the elements need", what, excess.tolist())


@pytest.mark.parametrize("E", (1, 2, 4, 8))
@pytest.mark.parametrize("filt", (BYTES, BITS), ids=("bytes", "bits"))
def test_the_ranges_are_exactly_the_bytes_the_elements_depend_on(E, filt):
    for n in SIZES:
        check_case(n, E, filt)


def test_the_interval_shortcut_of_the_check_is_the_exact_set():
    """check_case compares intervals; here the exact set, byte by byte, for sizes with a ragged end."""
    for E, n in ((2, 9), (1, 129), (8, 23)):
        for filt in (BYTES, BITS):
            for first, last in [(a, b) for a in range(n + 1) for b in range(a, n + 1)][::7]:
                got = ranges_of(n, E, filt, first, last)
                for (a, b), want in zip(got, needed(n, E, filt, first, last)):
                    assert list(range(a, b)) == want, (E, n, filt, first, last)


def test_bad_arguments_answer_no_ranges():
    assert ranges_of(100, 3, BYTES, 0, 10) == [] and ranges_of(100, 2, 2, 0, 10) == []
    assert ranges_of(100, 2, BYTES, 11, 10) == [] and ranges_of(100, 2, BYTES, 0, 101) == []
    assert ranges_of(100, 2, BYTES, 0, 10, room=1) == [] and ranges_of(100, 2, BITS, 0, 10, room=16) == []
    assert len(ranges_of(100, 2, BYTES, 0, 10, room=2)) == 2 and len(ranges_of(100, 2, BITS, 0, 10, room=17)) == 17
    assert lib().LizardGPU_planesRangeBytes(100, 2, BYTES, 0, 10, None, 65) == 0


def test_an_element_size_of_one_with_byte_planes_is_one_range():
    assert ranges_of(300000, 1, BYTES, 17, 4000) == [(17, 4000)]


def bound(ranges, B):
    arr = (Range * max(len(ranges), 1))(*[Range(a, b) for a, b in ranges])
    return lib().LizardGPU_frameRangesBound(arr, len(ranges), B)


def test_the_bound_is_the_obvious_sum():
    B = 131072
    rng = np.random.RandomState(3)
    cases = [[], [(0, 0)], [(5, 5)], [(0, 1)], [(0, B)], [(0, B + 1)], [(B - 1, B)], [(B - 1, B + 1)], [(B, 2 * B)], [(3 * B + 7, 5 * B)],
             [(B, B)], [(1, 2), (B - 1, B + 1), (7 * B, 7 * B), (2 * B, 3 * B)]]
    for _ in range(50):
        cases.append([tuple(sorted(int(v) for v in rng.randint(0, 10 * B, 2))) for _ in range(rng.randint(1, 9))])
    for ranges in cases:
        for bs in (B, 1, 4096):
            want = sum((-(-b // bs) - a // bs) * bs for a, b in ranges if b > a)
            assert bound(ranges, bs) == want, (ranges, bs)
    assert bound([(0, 10)], 0) == 0 and lib().LizardGPU_frameRangesBound(None, 1, B) == 0
    assert bound([(B - 1, B)], B) == B and bound([(0, 2 * B)], B) == 2 * B          # a range ending exactly on a block edge


def test_the_arithmetic_as_a_stand_alone_program_under_address_sanitizer():
    """tests/planes_range_asan_main.c: every (first, last) of small buffers and the bound, every array a heap allocation of exactly
    the entries the functions may touch."""
    if not util.sanitizer_runtime(_dir):
        pytest.skip("no AddressSanitizer runtime: a trivial program does not build with -fsanitize=address,undefined")
    exe = os.path.join(_dir, "planes_range_asan_main")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "planes_range_asan_main.c"), os.path.join(CSRC, "lizard_slice_host.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "planes_range_asan_main: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
