"""CPU: the tensor header of a tensor stream (LizardGPU_tensorHeaderWrite / LizardGPU_tensorHeaderRead, include/lizard_amd.h Part 3c):
a skippable frame that carries the element size a frame's bytes were split with, the dtype's name and the shape.  The bytes are the
documented ones, Read returns what Write was given, every documented refusal is refused, a cut at every prefix length is an incomplete
header, Write into too small a room writes nothing, and the reference's LizardF_decompress steps over a written header as over any
skippable frame."""
import ctypes as C
import os
import struct

import pytest

import util
from lizard_amd import _lib

MAGIC = 0x184D2A54
E_INCOMPLETE, E_UNKNOWN = 12, 13


class Desc(C.Structure):
    _fields_ = [("elemSize", C.c_uint32), ("ndim", C.c_uint32), ("nbytes", C.c_uint64), ("shape", C.c_uint64 * 8), ("dtype", C.c_char * 24)]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    L.LizardGPU_tensorHeaderWrite.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.LizardGPU_tensorHeaderWrite.restype = C.c_size_t
    L.LizardGPU_tensorHeaderRead.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.LizardGPU_tensorHeaderRead.restype = C.c_int
    return L


def desc(elem, shape, nbytes, dtype):
    d = Desc()
    d.elemSize, d.ndim, d.nbytes, d.dtype = elem, len(shape), nbytes, dtype
    for i, s in enumerate(shape[:8]):
        d.shape[i] = s
    return d


def documented(elem, shape, nbytes, dtype):
    """The header's bytes, assembled from the table in include/lizard_amd.h."""
    payload = b"LZT1" + bytes([elem, len(shape), 0, 0]) + struct.pack("<Q", nbytes) + dtype.ljust(24, b"\0") + b"".join(struct.pack("<Q", s) for s in shape)
    assert len(payload) == 40 + 8 * len(shape)
    return struct.pack("<II", MAGIC, len(payload)) + payload


def write(L, d, room=200):
    buf = C.create_string_buffer(b"\xEE" * (room + 1), room + 1)
    n = L.LizardGPU_tensorHeaderWrite(buf, room, C.byref(d))
    return n, buf.raw


def read(L, data, size=None):
    d, hb = Desc(), C.c_size_t(77)
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    rc = L.LizardGPU_tensorHeaderRead(buf, len(data) if size is None else size, C.byref(d), C.byref(hb))
    return rc, d, hb.value


CASES = [(2, (), 2, b"float16"), (4, (3,), 12, b"float32"), (8, (1, 2, 3, 4, 5, 6, 7, 2 ** 40), 8 * 5040 * 2 ** 40, b"int64"),
         (1, (1000, 37), 74000, b"bfloat16"), (1, (5,), 5, b"x" * 23)]


def test_the_descriptor_is_the_one_the_header_file_declares():
    assert C.sizeof(Desc) == 4 + 4 + 8 + 64 + 24


def test_write_then_read_round_trip_and_the_documented_bytes(lib):
    assert {len(c[1]) for c in CASES} >= {0, 1, 8}
    for elem, shape, nbytes, dtype in CASES:
        n, raw = write(lib, desc(elem, shape, nbytes, dtype))
        want = documented(elem, shape, nbytes, dtype)
        assert n == len(want) == 48 + 8 * len(shape) and raw[:n] == want
        assert raw[n:] == b"\xEE" * (len(raw) - n), "Write wrote behind the header"
        for tail in (b"", b"\x04\x22\x4D\x18 and what follows"):
            rc, d, hb = read(lib, want + tail)
            assert rc == 0 and hb == n
            assert (d.elemSize, d.ndim, d.nbytes, d.dtype, tuple(d.shape[:d.ndim])) == (elem, len(shape), nbytes, dtype, shape)
            assert all(s == 0 for s in d.shape[d.ndim:])
        # either output may be NULL
        buf = C.create_string_buffer(want, len(want))
        assert lib.LizardGPU_tensorHeaderRead(buf, len(want), None, None) == 0


def test_a_cut_at_every_prefix_length_is_an_incomplete_header(lib):
    for elem, shape, nbytes, dtype in CASES:
        want = documented(elem, shape, nbytes, dtype)
        for k in range(len(want)):
            rc, _, hb = read(lib, want[:k])
            assert rc == -E_INCOMPLETE and hb == 0, (dtype, k, rc)


def test_every_documented_refusal(lib):
    good = documented(4, (3, 5), 60, b"float32")
    assert read(lib, good)[0] == 0

    def patched(at, new):
        return good[:at] + new + good[at + len(new):]
    bad = {
        "a data frame's magic": patched(0, struct.pack("<I", 0x184D2206)),
        "another skippable magic": patched(0, struct.pack("<I", 0x184D2A57)),
        "a wrong tag": patched(8, b"LZT2"),
        "a length that is no header's": patched(4, struct.pack("<I", 40 + 8 * 2 + 1)),
        "a length below the fixed part": patched(4, struct.pack("<I", 32)),
        "a length for nine dims": patched(4, struct.pack("<I", 40 + 72)) + bytes(80),
        "ndim that disagrees with the length": patched(13, b"\x03"),
        "ndim above eight": patched(13, b"\x09"),
        "a non-zero first pad byte": patched(14, b"\x01"),
        "a non-zero second pad byte": patched(15, b"\x01"),
        "element size 0": patched(12, b"\x00"),
        "element size 3": patched(12, b"\x03"),
        "element size 16": patched(12, b"\x10"),
        "a dtype name that fills its field": patched(24, b"n" * 24),
    }
    for what, data in bad.items():
        rc, _, hb = read(lib, data)
        assert rc == -E_UNKNOWN and hb == 0, (what, rc)
    # a foreign skippable frame, whole
    assert read(lib, struct.pack("<II", 0x184D2A57, 9) + b"skippable")[0] == -E_UNKNOWN
    # Write refuses what Read would refuse, and writes nothing
    for d in (desc(3, (1,), 3, b"int8"), desc(0, (1,), 1, b"int8"), desc(16, (1,), 16, b"complex128"), desc(4, (1,) * 9, 4, b"float32")):
        n, raw = write(lib, d)
        assert n == 0 and raw == b"\xEE" * len(raw)
    d = desc(4, (1,), 4, b"float32")
    C.memmove(C.addressof(d) + Desc.dtype.offset, b"n" * 24, 24)
    n, raw = write(lib, d)
    assert n == 0 and raw == b"\xEE" * len(raw)


def test_write_into_one_byte_too_little_writes_nothing(lib):
    for elem, shape, nbytes, dtype in CASES:
        need = 48 + 8 * len(shape)
        n, raw = write(lib, desc(elem, shape, nbytes, dtype), room=need - 1)
        assert n == 0 and raw == b"\xEE" * need, "the byte behind the capacity, or one in front of it, changed"
        n, raw = write(lib, desc(elem, shape, nbytes, dtype), room=need)
        assert n == need and raw[need:] == b"\xEE"


def test_the_reference_frame_decoder_steps_over_a_written_header(lib):
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
        n, raw = write(lib, desc(elem, shape, nbytes, dtype))
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
