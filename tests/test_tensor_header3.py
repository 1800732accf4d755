"""CPU: the tensor header of a tensor that was XORed with a base (LizardGPU_tensorHeaderWrite3 / LizardGPU_tensorHeaderRead3,
include/lizard_amd.h Part 3c).  Write3 with flags 0 writes exactly Write2's bytes ("LZT1" / "LZT2") and refuses a base tag then; with
flags 1 the "LZT2" layout under the tag "LZT3" with payload byte 6 = the filter, byte 7 = 1, the base tag at payload 40 .. 47 and the
dims from 48; any other flags write nothing.  Read3 gives back what Write3 was given for all three tags, Read and Read2 refuse
"LZT3", every documented refusal is refused, a cut at every prefix length is an incomplete header, Write3 into too small a room
writes nothing, and the reference's LizardF_decompress steps over an "LZT3" header as over any skippable frame."""
import ctypes as C
import os
import struct

import pytest

import util
from lizard_amd import _lib

MAGIC = 0x184D2A54
E_INCOMPLETE, E_UNKNOWN = 12, 13
BYTES, BITS = 0, 1
XOR_BASE = 1


class Desc(C.Structure):
    _fields_ = [("elemSize", C.c_uint32), ("ndim", C.c_uint32), ("nbytes", C.c_uint64), ("shape", C.c_uint64 * 8), ("dtype", C.c_char * 24)]


class Desc2(C.Structure):
    _fields_ = Desc._fields_ + [("filter", C.c_uint32), ("reserved", C.c_uint32)]


class Desc3(C.Structure):
    _fields_ = Desc._fields_ + [("filter", C.c_uint32), ("flags", C.c_uint32), ("baseTag", C.c_uint64)]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("LizardGPU_tensorHeaderWrite", "LizardGPU_tensorHeaderWrite2", "LizardGPU_tensorHeaderWrite3"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        getattr(L, name).restype = C.c_size_t
    for name in ("LizardGPU_tensorHeaderRead", "LizardGPU_tensorHeaderRead2", "LizardGPU_tensorHeaderRead3"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        getattr(L, name).restype = C.c_int
    return L


def desc3(elem, shape, nbytes, dtype, filt, flags, tag):
    d = Desc3()
    d.elemSize, d.ndim, d.nbytes, d.dtype, d.filter, d.flags, d.baseTag = elem, len(shape), nbytes, dtype, filt, flags, tag
    for i, s in enumerate(shape[:8]):
        d.shape[i] = s
    return d


def desc2(elem, shape, nbytes, dtype, filt):
    d = Desc2()
    d.elemSize, d.ndim, d.nbytes, d.dtype, d.filter = elem, len(shape), nbytes, dtype, filt
    for i, s in enumerate(shape[:8]):
        d.shape[i] = s
    return d


def documented(elem, shape, nbytes, dtype, filt, flags=0, tag=0):
    """The header's bytes, assembled from the tables in include/lizard_amd.h."""
    if flags:
        payload = (b"LZT3" + bytes([elem, len(shape), filt, flags]) + struct.pack("<Q", nbytes) + dtype.ljust(24, b"\0")
                   + struct.pack("<Q", tag) + b"".join(struct.pack("<Q", s) for s in shape))
        assert len(payload) == 48 + 8 * len(shape)
    else:
        payload = ((b"LZT2" if filt else b"LZT1") + bytes([elem, len(shape), filt, 0]) + struct.pack("<Q", nbytes) + dtype.ljust(24, b"\0")
                   + b"".join(struct.pack("<Q", s) for s in shape))
        assert len(payload) == 40 + 8 * len(shape)
    return struct.pack("<II", MAGIC, len(payload)) + payload


def write(fn, d, room=200):
    buf = C.create_string_buffer(b"\xEE" * (room + 1), room + 1)
    n = fn(buf, room, C.byref(d))
    return n, buf.raw


def read3(L, data, size=None):
    d, hb = Desc3(), C.c_size_t(77)
    d.filter, d.flags, d.baseTag = 99, 99, 99
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    rc = L.LizardGPU_tensorHeaderRead3(buf, len(data) if size is None else size, C.byref(d), C.byref(hb))
    return rc, d, hb.value


def read_old(L, name, data):
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    hb = C.c_size_t(77)
    return getattr(L, name)(buf, len(data), C.byref(Desc2()), C.byref(hb)), hb.value


CASES = [(2, (), 2, b"float16"), (4, (3,), 12, b"float32"), (8, (1, 2, 3, 4, 5, 6, 7, 2 ** 40), 8 * 5040 * 2 ** 40, b"int64"),
         (1, (1000, 37), 74000, b"bfloat16"), (1, (5,), 5, b"x" * 23)]
TAGS = (0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1)
# (filter, flags): "LZT1", "LZT2", "LZT3" over byte planes, "LZT3" over bit planes
KINDS = ((BYTES, 0), (BITS, 0), (BYTES, XOR_BASE), (BITS, XOR_BASE))


def test_the_descriptor_is_the_v2_fields_with_flags_then_the_base_tag():
    assert C.sizeof(Desc3) == 120 and C.sizeof(Desc2) == 112
    assert all(getattr(Desc3, n).offset == getattr(Desc2, n).offset for n, _ in Desc2._fields_ if n != "reserved")
    assert Desc3.filter.offset == 104 and Desc3.flags.offset == 108 == Desc2.reserved.offset and Desc3.baseTag.offset == 112


def test_write3_with_flags_0_is_byte_identical_to_write2_and_refuses_a_base_tag(lib):
    for filt in (BYTES, BITS):
        for elem, shape, nbytes, dtype in CASES:
            n2, raw2 = write(lib.LizardGPU_tensorHeaderWrite2, desc2(elem, shape, nbytes, dtype, filt))
            n3, raw3 = write(lib.LizardGPU_tensorHeaderWrite3, desc3(elem, shape, nbytes, dtype, filt, 0, 0))
            assert n2 == n3 == 48 + 8 * len(shape) and raw2 == raw3 and raw3[:n3] == documented(elem, shape, nbytes, dtype, filt)
            assert raw3[8:12] == (b"LZT2" if filt else b"LZT1")
            n, raw = write(lib.LizardGPU_tensorHeaderWrite3, desc3(elem, shape, nbytes, dtype, filt, 0, 5))
            assert n == 0 and raw == b"\xEE" * len(raw), "a base tag without a base was written"


def test_the_documented_lzt3_bytes_and_the_round_trip_for_all_three_tags(lib):
    assert {len(c[1]) for c in CASES} >= {0, 1, 8}
    for filt, flags in KINDS:
        for k, (elem, shape, nbytes, dtype) in enumerate(CASES):
            tag = TAGS[k % len(TAGS)] if flags else 0
            n, raw = write(lib.LizardGPU_tensorHeaderWrite3, desc3(elem, shape, nbytes, dtype, filt, flags, tag))
            want = documented(elem, shape, nbytes, dtype, filt, flags, tag)
            assert n == len(want) == (56 if flags else 48) + 8 * len(shape) and raw[:n] == want
            assert raw[n:] == b"\xEE" * (len(raw) - n), "Write3 wrote behind the header"
            if flags:
                assert want[8:12] == b"LZT3" and want[8 + 6] == filt and want[8 + 7] == 1
                assert want[8 + 40:8 + 48] == struct.pack("<Q", tag) and struct.unpack("<I", want[4:8])[0] == 48 + 8 * len(shape)
            for tail in (b"", b"\x04\x22\x4D\x18 and what follows"):
                rc, d, hb = read3(lib, want + tail)
                assert rc == 0 and hb == n
                assert (d.elemSize, d.ndim, d.nbytes, d.dtype, tuple(d.shape[:d.ndim])) == (elem, len(shape), nbytes, dtype, shape)
                assert all(s == 0 for s in d.shape[d.ndim:])
                assert (d.filter, d.flags, d.baseTag) == (filt, flags, tag)
            buf = C.create_string_buffer(want, len(want))        # either output may be NULL
            assert lib.LizardGPU_tensorHeaderRead3(buf, len(want), None, None) == 0


def test_read_and_read2_refuse_lzt3_and_read3_reads_what_write_and_write2_make(lib):
    for elem, shape, nbytes, dtype in CASES:
        for filt in (BYTES, BITS):
            lzt3 = documented(elem, shape, nbytes, dtype, filt, XOR_BASE, 7)
            assert read_old(lib, "LizardGPU_tensorHeaderRead", lzt3) == (-E_UNKNOWN, 0)
            assert read_old(lib, "LizardGPU_tensorHeaderRead2", lzt3) == (-E_UNKNOWN, 0)
            n, raw = write(lib.LizardGPU_tensorHeaderWrite2, desc2(elem, shape, nbytes, dtype, filt))
            rc, d, hb = read3(lib, raw[:n])
            assert rc == 0 and hb == n and (d.filter, d.flags, d.baseTag) == (filt, 0, 0)


def test_a_cut_at_every_prefix_length_is_an_incomplete_header(lib):
    for filt, flags in KINDS:
        for elem, shape, nbytes, dtype in CASES:
            want = documented(elem, shape, nbytes, dtype, filt, flags, 0xFEDCBA9876543210 if flags else 0)
            for k in range(len(want)):
                rc, d, hb = read3(lib, want[:k])
                assert rc == -E_INCOMPLETE and hb == 0, (filt, flags, dtype, k, rc)
                assert d.filter == 99 and d.flags == 99 and d.baseTag == 99, "a refused read wrote the descriptor"


def test_every_documented_refusal(lib):
    for filt in (BYTES, BITS):
        good = documented(4, (3, 5), 60, b"float32", filt, XOR_BASE, 9)
        assert read3(lib, good)[0] == 0

        def patched(at, new):
            return good[:at] + new + good[at + len(new):]
        bad = {
            "a data frame's magic": patched(0, struct.pack("<I", 0x184D2206)),
            "another skippable magic": patched(0, struct.pack("<I", 0x184D2A57)),
            "a tag this reader does not know": patched(8, b"LZT4"),
            "a tag of another case": patched(8, b"lzt3"),
            "a length that is no header's": patched(4, struct.pack("<I", 48 + 8 * 2 + 1)),
            "a length below every fixed part": patched(4, struct.pack("<I", 32)),
            "a length below this tag's fixed part": patched(4, struct.pack("<I", 40))[:48],
            "a length for nine dims": patched(4, struct.pack("<I", 48 + 72)) + bytes(80),
            "ndim that disagrees with the length": patched(13, b"\x03"),
            "ndim counted from the v2 fixed part": patched(13, b"\x03"),
            "ndim above eight": patched(13, b"\x09"),
            "filter 2": patched(14, b"\x02"),
            "filter 255": patched(14, b"\xFF"),
            "flags 0 under LZT3": patched(15, b"\x00"),
            "flags 2": patched(15, b"\x02"),
            "flags 3": patched(15, b"\x03"),
            "element size 0": patched(12, b"\x00"),
            "element size 3": patched(12, b"\x03"),
            "element size 16": patched(12, b"\x10"),
            "a dtype name that fills its field": patched(24, b"n" * 24),
        }
        for what, data in bad.items():
            rc, d, hb = read3(lib, data)
            assert rc == -E_UNKNOWN and hb == 0 and d.filter == 99, (filt, what, rc)
        # one encoding per meaning: flags under "LZT1" / "LZT2" are no headers, and "LZT2" keeps its one filter
        plain = documented(4, (3, 5), 60, b"float32", filt)
        assert read3(lib, plain[:15] + b"\x01" + plain[16:])[0] == -E_UNKNOWN
        assert read3(lib, plain[:8] + b"LZT2" + plain[12:14] + b"\0\0" + plain[16:])[0] == -E_UNKNOWN
        assert read3(lib, plain[:8] + b"LZT1" + plain[12:14] + b"\1\0" + plain[16:])[0] == -E_UNKNOWN
        # a v2 header whose length only an "LZT3" header may have (ndim would be 9 from the v2 fixed part)
        long2 = documented(4, (1,) * 8, 4, b"float32", filt)
        assert read3(lib, long2[:4] + struct.pack("<I", 112) + long2[8:] + bytes(8))[0] == -E_UNKNOWN
    # a foreign skippable frame, whole
    assert read3(lib, struct.pack("<II", 0x184D2A57, 9) + b"skippable")[0] == -E_UNKNOWN
    # Write3 refuses what Read3 would refuse, any flags and any filter it does not know, and writes nothing
    refused = [desc3(3, (1,), 3, b"int8", BITS, 1, 0), desc3(0, (1,), 1, b"int8", BYTES, 1, 0), desc3(16, (1,), 16, b"complex128", BITS, 1, 0),
               desc3(4, (1,) * 9, 4, b"float32", BITS, 1, 0), desc3(4, (1,), 4, b"float32", 2, 1, 0), desc3(4, (1,), 4, b"float32", 256, 1, 0),
               desc3(4, (1,), 4, b"float32", 2, 0, 0), desc3(4, (1,), 4, b"float32", BYTES, 2, 0), desc3(4, (1,), 4, b"float32", BITS, 3, 1),
               desc3(4, (1,), 4, b"float32", BYTES, 257, 0), desc3(4, (1,), 4, b"float32", BYTES, 0xFFFFFFFF, 0)]
    for d in refused:
        n, raw = write(lib.LizardGPU_tensorHeaderWrite3, d)
        assert n == 0 and raw == b"\xEE" * len(raw)
    d = desc3(4, (1,), 4, b"float32", BITS, 1, 0)
    C.memmove(C.addressof(d) + Desc3.dtype.offset, b"n" * 24, 24)
    n, raw = write(lib.LizardGPU_tensorHeaderWrite3, d)
    assert n == 0 and raw == b"\xEE" * len(raw)
    d = desc3(4, (1,), 4, b"float32", BITS, 1, 0)
    buf = C.create_string_buffer(b"\xEE" * 200, 200)
    assert lib.LizardGPU_tensorHeaderWrite3(buf, 200, None) == 0 and lib.LizardGPU_tensorHeaderWrite3(None, 200, C.byref(d)) == 0
    assert buf.raw == b"\xEE" * 200


def test_a_short_prefix_accepts_a_length_of_any_tag_and_the_tag_then_decides(lib):
    """With fewer than 12 bytes a length is accepted when some tag has it; 112 is an "LZT3" length only, 40 an "LZT1" / "LZT2" one."""
    for length, tags in ((112, (b"LZT3",)), (40, (b"LZT1", b"LZT2")), (48, (b"LZT1", b"LZT2", b"LZT3"))):
        head = struct.pack("<II", MAGIC, length)
        assert read3(lib, head)[0] == -E_INCOMPLETE
        for tag in (b"LZT1", b"LZT2", b"LZT3"):
            assert read3(lib, head + tag)[0] == (-E_INCOMPLETE if tag in tags else -E_UNKNOWN), (length, tag)
    assert read3(lib, struct.pack("<II", MAGIC, 120))[0] == -E_UNKNOWN
    assert read_old(lib, "LizardGPU_tensorHeaderRead2", struct.pack("<II", MAGIC, 112))[0] == -E_UNKNOWN   # the old readers' bound stays


def test_write3_into_one_byte_too_little_writes_nothing(lib):
    for filt, flags in KINDS:
        for elem, shape, nbytes, dtype in CASES:
            need = (56 if flags else 48) + 8 * len(shape)
            n, raw = write(lib.LizardGPU_tensorHeaderWrite3, desc3(elem, shape, nbytes, dtype, filt, flags, 3 * flags), room=need - 1)
            assert n == 0 and raw == b"\xEE" * need, "the byte behind the capacity, or one in front of it, changed"
            n, raw = write(lib.LizardGPU_tensorHeaderWrite3, desc3(elem, shape, nbytes, dtype, filt, flags, 3 * flags), room=need)
            assert n == need and raw[need:] == b"\xEE"


def test_the_reference_frame_decoder_steps_over_an_lzt3_header(lib):
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
        n, raw = write(lib.LizardGPU_tensorHeaderWrite3, desc3(elem, shape, nbytes, dtype, BITS, XOR_BASE, 2 ** 63 + 5))
        assert raw[8:12] == b"LZT3"
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
