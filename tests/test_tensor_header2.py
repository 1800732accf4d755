"""CPU: the tensor header with a filter (LizardGPU_tensorHeaderWrite2 / LizardGPU_tensorHeaderRead2, include/lizard_amd.h Part 3c).
Write2 with the byte-plane filter writes exactly LizardGPU_tensorHeaderWrite's "LZT1" bytes; with the bit-plane filter the same layout
under the tag "LZT2", payload byte 6 = 1 and byte 7 = 0; any other filter writes nothing.  Read2 gives back what Write2 was given for
both tags, the old Read still refuses "LZT2", every documented refusal is refused, a cut at every prefix length is an incomplete
header, Write2 into too small a room writes nothing, and the reference's LizardF_decompress steps over an "LZT2" header as over any
skippable frame."""
import ctypes as C
import os
import struct

import pytest

import util
from lizard_amd import _lib

MAGIC = 0x184D2A54
E_INCOMPLETE, E_UNKNOWN = 12, 13
BYTES, BITS = 0, 1


class Desc(C.Structure):
    _fields_ = [("elemSize", C.c_uint32), ("ndim", C.c_uint32), ("nbytes", C.c_uint64), ("shape", C.c_uint64 * 8), ("dtype", C.c_char * 24)]


class Desc2(C.Structure):
    _fields_ = Desc._fields_ + [("filter", C.c_uint32), ("reserved", C.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("LizardGPU_tensorHeaderWrite", "LizardGPU_tensorHeaderWrite2"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        getattr(L, name).restype = C.c_size_t
    for name in ("LizardGPU_tensorHeaderRead", "LizardGPU_tensorHeaderRead2"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        getattr(L, name).restype = C.c_int
    return L


def desc(elem, shape, nbytes, dtype, filt=None, reserved=0):
    d = Desc() if filt is None else Desc2()
    d.elemSize, d.ndim, d.nbytes, d.dtype = elem, len(shape), nbytes, dtype
    for i, s in enumerate(shape[:8]):
        d.shape[i] = s
    if filt is not None:
        d.filter, d.reserved = filt, reserved
    return d


def documented(elem, shape, nbytes, dtype, filt):
    """The header's bytes, assembled from the table in include/lizard_amd.h."""
    payload = ((b"LZT2" if filt else b"LZT1") + bytes([elem, len(shape), filt, 0]) + struct.pack("<Q", nbytes) + dtype.ljust(24, b"\0")
               + b"".join(struct.pack("<Q", s) for s in shape))
    assert len(payload) == 40 + 8 * len(shape)
    return struct.pack("<II", MAGIC, len(payload)) + payload


def write(fn, d, room=200):
    buf = C.create_string_buffer(b"\xEE" * (room + 1), room + 1)
    n = fn(buf, room, C.byref(d))
    return n, buf.raw


def read2(L, data, size=None):
    d, hb = Desc2(), C.c_size_t(77)
    d.filter, d.reserved = 99, 99
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    rc = L.LizardGPU_tensorHeaderRead2(buf, len(data) if size is None else size, C.byref(d), C.byref(hb))
    return rc, d, hb.value


def read1(L, data):
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    hb = C.c_size_t(77)
    return L.LizardGPU_tensorHeaderRead(buf, len(data), C.byref(Desc()), C.byref(hb)), hb.value


CASES = [(2, (), 2, b"float16"), (4, (3,), 12, b"float32"), (8, (1, 2, 3, 4, 5, 6, 7, 2 ** 40), 8 * 5040 * 2 ** 40, b"int64"),
         (1, (1000, 37), 74000, b"bfloat16"), (1, (5,), 5, b"x" * 23)]


def test_the_descriptor_is_the_v1_fields_then_filter_and_reserved():
    assert C.sizeof(Desc) == 104 and C.sizeof(Desc2) == 112
    assert all(getattr(Desc2, n).offset == getattr(Desc, n).offset for n, _ in Desc._fields_)
    assert Desc2.filter.offset == 104 and Desc2.reserved.offset == 108


def test_write2_with_byte_planes_is_byte_identical_to_write(lib):
    for elem, shape, nbytes, dtype in CASES:
        n1, raw1 = write(lib.LizardGPU_tensorHeaderWrite, desc(elem, shape, nbytes, dtype))
        n2, raw2 = write(lib.LizardGPU_tensorHeaderWrite2, desc(elem, shape, nbytes, dtype, BYTES, reserved=0xDEAD))
        assert n1 == n2 == 48 + 8 * len(shape) and raw1 == raw2 and raw2[:n2] == documented(elem, shape, nbytes, dtype, BYTES)
        assert raw2[8:12] == b"LZT1"


def test_the_documented_lzt2_bytes_and_the_round_trip_for_both_tags(lib):
    assert {len(c[1]) for c in CASES} >= {0, 1, 8}
    for filt in (BYTES, BITS):
        for elem, shape, nbytes, dtype in CASES:
            n, raw = write(lib.LizardGPU_tensorHeaderWrite2, desc(elem, shape, nbytes, dtype, filt, reserved=7))
            want = documented(elem, shape, nbytes, dtype, filt)
            assert n == len(want) == 48 + 8 * len(shape) and raw[:n] == want
            assert raw[n:] == b"\xEE" * (len(raw) - n), "Write2 wrote behind the header"
            if filt == BITS:
                assert want[8:12] == b"LZT2" and want[8 + 6] == 1 and want[8 + 7] == 0
            for tail in (b"", b"\x04\x22\x4D\x18 and what follows"):
                rc, d, hb = read2(lib, want + tail)
                assert rc == 0 and hb == n
                assert (d.elemSize, d.ndim, d.nbytes, d.dtype, tuple(d.shape[:d.ndim])) == (elem, len(shape), nbytes, dtype, shape)
                assert all(s == 0 for s in d.shape[d.ndim:])
                assert d.filter == filt and d.reserved == 0
            buf = C.create_string_buffer(want, len(want))        # either output may be NULL
            assert lib.LizardGPU_tensorHeaderRead2(buf, len(want), None, None) == 0


def test_the_old_reader_still_refuses_lzt2_and_reads_what_write2_makes_of_byte_planes(lib):
    for elem, shape, nbytes, dtype in CASES:
        assert read1(lib, documented(elem, shape, nbytes, dtype, BITS)) == (-E_UNKNOWN, 0)
        assert read1(lib, documented(elem, shape, nbytes, dtype, BYTES)) == (0, 48 + 8 * len(shape))
        lzt2_filter0 = documented(elem, shape, nbytes, dtype, BITS)[:14] + b"\0" + documented(elem, shape, nbytes, dtype, BITS)[15:]
        assert read1(lib, lzt2_filter0) == (-E_UNKNOWN, 0)


def test_a_cut_at_every_prefix_length_is_an_incomplete_header(lib):
    for filt in (BYTES, BITS):
        for elem, shape, nbytes, dtype in CASES:
            want = documented(elem, shape, nbytes, dtype, filt)
            for k in range(len(want)):
                rc, d, hb = read2(lib, want[:k])
                assert rc == -E_INCOMPLETE and hb == 0, (filt, dtype, k, rc)
                assert d.filter == 99, "a refused read wrote the descriptor"


def test_every_documented_refusal(lib):
    for filt in (BYTES, BITS):
        good = documented(4, (3, 5), 60, b"float32", filt)
        assert read2(lib, good)[0] == 0

        def patched(at, new):
            return good[:at] + new + good[at + len(new):]
        bad = {
            "a data frame's magic": patched(0, struct.pack("<I", 0x184D2206)),
            "another skippable magic": patched(0, struct.pack("<I", 0x184D2A57)),
            "a wrong tag": patched(8, b"LZT3"),
            "a tag of another case": patched(8, b"lzt2"),
            "a length that is no header's": patched(4, struct.pack("<I", 40 + 8 * 2 + 1)),
            "a length below the fixed part": patched(4, struct.pack("<I", 32)),
            "a length for nine dims": patched(4, struct.pack("<I", 40 + 72)) + bytes(80),
            "ndim that disagrees with the length": patched(13, b"\x03"),
            "ndim above eight": patched(13, b"\x09"),
            "a filter byte that is not the tag's": patched(14, bytes([1 - filt])),
            "filter 2": patched(14, b"\x02"),
            "a non-zero byte 7": patched(15, b"\x01"),
            "element size 0": patched(12, b"\x00"),
            "element size 3": patched(12, b"\x03"),
            "element size 16": patched(12, b"\x10"),
            "a dtype name that fills its field": patched(24, b"n" * 24),
        }
        for what, data in bad.items():
            rc, d, hb = read2(lib, data)
            assert rc == -E_UNKNOWN and hb == 0 and d.filter == 99, (filt, what, rc)
        # one encoding per meaning: byte planes under "LZT2" and bit planes under "LZT1" are no headers
        assert read2(lib, documented(4, (3, 5), 60, b"float32", BYTES)[:8] + b"LZT2" + good[12:14] + b"\0\0" + good[16:])[0] == -E_UNKNOWN
        assert read2(lib, documented(4, (3, 5), 60, b"float32", BYTES)[:8] + b"LZT1" + good[12:14] + b"\1\0" + good[16:])[0] == -E_UNKNOWN
    # a foreign skippable frame, whole
    assert read2(lib, struct.pack("<II", 0x184D2A57, 9) + b"skippable")[0] == -E_UNKNOWN
    # Write2 refuses what Read2 would refuse, and any filter it does not know, and writes nothing
    refused = [desc(3, (1,), 3, b"int8", BITS), desc(0, (1,), 1, b"int8", BYTES), desc(16, (1,), 16, b"complex128", BITS),
               desc(4, (1,) * 9, 4, b"float32", BITS), desc(4, (1,), 4, b"float32", 2), desc(4, (1,), 4, b"float32", 256),
               desc(4, (1,), 4, b"float32", 257), desc(4, (1,), 4, b"float32", 0xFFFFFFFF)]
    for d in refused:
        n, raw = write(lib.LizardGPU_tensorHeaderWrite2, d)
        assert n == 0 and raw == b"\xEE" * len(raw)
    d = desc(4, (1,), 4, b"float32", BITS)
    C.memmove(C.addressof(d) + Desc2.dtype.offset, b"n" * 24, 24)
    n, raw = write(lib.LizardGPU_tensorHeaderWrite2, d)
    assert n == 0 and raw == b"\xEE" * len(raw)
    buf = C.create_string_buffer(b"\xEE" * 200, 200)
    assert lib.LizardGPU_tensorHeaderWrite2(buf, 200, None) == 0 and lib.LizardGPU_tensorHeaderWrite2(None, 200, C.byref(d)) == 0
    assert buf.raw == b"\xEE" * 200


def test_write2_into_one_byte_too_little_writes_nothing(lib):
    for filt in (BYTES, BITS):
        for elem, shape, nbytes, dtype in CASES:
            need = 48 + 8 * len(shape)
            n, raw = write(lib.LizardGPU_tensorHeaderWrite2, desc(elem, shape, nbytes, dtype, filt), room=need - 1)
            assert n == 0 and raw == b"\xEE" * need, "the byte behind the capacity, or one in front of it, changed"
            n, raw = write(lib.LizardGPU_tensorHeaderWrite2, desc(elem, shape, nbytes, dtype, filt), room=need)
            assert n == need and raw[need:] == b"\xEE"


def test_the_reference_frame_decoder_steps_over_an_lzt2_header(lib):
    util.reference()                                             # builds oracle/_ref where the reference's sources are present
    path = os.path.join(util.REF_DIR, "liblizard_ref.so")
    if not os.path.exists(path):
        util.need_ref("oracle/_ref/liblizard_ref.so")
    R = C.CDLL(path)
    R.LizardF_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]
    R.LizardF_createDecompressionContext.restype = C.c_size_t
    R.LizardF_decompress.restype = C.c_size_t
    R.LizardF_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    R.LizardF_freeDecompressionContext.argtypes = [C.c_void_p]
    for elem, shape, nbytes, dtype in CASES:
        n, raw = write(lib.LizardGPU_tensorHeaderWrite2, desc(elem, shape, nbytes, dtype, BITS))
        assert raw[8:12] == b"LZT2"
        dctx = C.c_void_p()
        assert R.LizardF_createDecompressionContext(C.byref(dctx), 100) == 0
        src, dst = C.create_string_buffer(raw[:n], n), C.create_string_buffer(64)
        pos, out, r = 0, 0, 1
        while pos < n:
            ds, ss = C.c_size_t(64), C.c_size_t(n - pos)
            r = R.LizardF_decompress(dctx, dst, C.byref(ds), C.byref(src, pos), C.byref(ss), None)
            assert r < (1 << 63), "the reference's frame decoder refused the header"
            assert ss.value > 0
            pos += ss.value
            out += ds.value
        assert (pos, out, r) == (n, 0, 0), "a skippable frame: every byte consumed, nothing decoded, the decoder at a frame's start again"
        R.LizardF_freeDecompressionContext(dctx)
