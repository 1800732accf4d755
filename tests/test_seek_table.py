"""CPU: the seek table codec (lizard_amd/csrc/lizard_seek_host.c; the format: include/lizard_amd.h Part 3b) against a model written with
struct (tests/seek_inputs.py): round trips for 1, 2 and 1 000 items, one damaged variant per rule of "usable" (never usable), the
"give me more tail" answer and then success, every truncation of a 3-item stream's tail, the codec as a stand-alone program under
AddressSanitizer + UBSan, and what the table is FOR every other reader of the format: frames + table decode to the frames' bytes in
the library's host LizardF_decompress and in the reference's."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import seek_inputs as si

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(util.ROOT, "lizard_amd", "csrc")
_dir = tempfile.mkdtemp(prefix="seek_table_")


class Entry(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("decodedBytes", C.c_uint64), ("prefixBytes", C.c_uint32), ("flags", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def lib():
    from lizard_amd import _lib
    _lib.build()
    return _lib.lib()


def write(entries):
    L = lib()
    n = len(entries)
    arr = (Entry * max(n, 1))(*[Entry(*e) for e in entries])
    cap = L.LizardGPU_seekTableBytes(n)
    buf = C.create_string_buffer(cap + 8)
    got = L.LizardGPU_seekTableWrite(buf, cap, arr, n)
    assert buf.raw[cap:] == b"\0" * 8
    return buf.raw[:got]


def read(tail, stream_bytes, room=None):
    """(answer, n, tableOffset, entries as 4-tuples) of LizardGPU_seekTableRead over `tail`, the last bytes of a stream."""
    L = lib()
    room = len(tail) // 24 + 1 if room is None else room
    arr, n, at = (Entry * max(room, 1))(), C.c_size_t(99), C.c_uint64(99)
    rc = L.LizardGPU_seekTableRead(bytes(tail), len(tail), stream_bytes, arr, room, C.byref(n), C.byref(at))
    return rc, n.value, at.value, [(e.offset, e.decodedBytes, e.prefixBytes, e.flags) for e in arr[:min(n.value, room)]]


def items(n):
    """n items that tile [0, end): every third without a prefix, one that decodes to nothing."""
    out, pos = [], 0
    for i in range(n):
        pre = 0 if i % 3 == 0 else 56 + 8 * (i % 5)
        out.append((pos, 0 if i == 1 else 1000003 * i + 1, pre, 0))
        pos += pre + 19 + i % 7
    return out, pos


def test_the_entry_is_24_bytes_and_the_sizes_are_the_formats():
    L = lib()
    assert C.sizeof(Entry) == 24
    assert [L.LizardGPU_seekTableBytes(n) for n in (0, 1, 2, 1000)] == [24, 48, 72, 24024]
    assert L.LizardGPU_seekTableBytes(178956969) == 24 * 178956969 + 24            # 24 n + 16 <= 2^32 - 1
    bad = L.LizardGPU_seekTableBytes(178956970)
    assert L.LizardGPU_frameIsError(bad) and (1 << 64) - bad == 1


@pytest.mark.parametrize("n", (1, 2, 1000))
def test_round_trip_against_the_struct_model(n):
    entries, end = items(n)
    table = write(entries)
    assert table == si.pack_table(entries) and len(table) == si.table_bytes(n)
    rc, got, at, back = read(table, end + len(table))
    assert (rc, got, at, back) == (si.USABLE, n, end, entries)
    # a longer tail than the table: frames' bytes in front of it are not looked at
    assert read(b"\xA5" * 100 + table, end + len(table))[:3] == (si.USABLE, n, end) if end >= 100 else True
    # an array shorter than the table: the first entries, the whole count
    rc, got, at, back = read(table, end + len(table), room=n // 2)
    assert (rc, got, at, back) == (si.USABLE, n, end, entries[:n // 2])
    # no room for the table: nothing is written
    L = lib()
    buf = C.create_string_buffer(b"\x5A" * len(table), len(table))
    assert L.LizardGPU_seekTableWrite(buf, len(table) - 1, (Entry * n)(*[Entry(*e) for e in entries]), n) == 0 and buf.raw == b"\x5A" * len(table)


def test_the_codec_needs_no_entries_array():
    entries, end = items(5)
    table = write(entries)
    n, at = C.c_size_t(0), C.c_uint64(0)
    assert lib().LizardGPU_seekTableRead(table, len(table), end + len(table), None, 0, C.byref(n), C.byref(at)) == si.USABLE
    assert (n.value, at.value) == (5, end)
    assert lib().LizardGPU_seekTableRead(table, len(table), len(table) - 1, None, 0, C.byref(n), C.byref(at)) == -3       # more tail than stream
    assert lib().LizardGPU_seekTableRead(None, 0, 100, None, 0, C.byref(n), C.byref(at)) == -3


def seekable_model_stream():
    """Five items of arbitrary bytes (the codec never looks at them) and their table."""
    entries, end = items(5)
    return bytes((7 * i) & 0xFF for i in range(end)) + si.pack_table(entries), entries, end


@pytest.mark.parametrize("name", si.DAMAGED_NAMES)
def test_a_damaged_table_is_never_usable(name):
    stream, entries, end = seekable_model_stream()
    assert read(stream[-si.table_bytes(5):], len(stream))[0] == si.USABLE
    bad = dict(si.damaged(stream))[name]
    for tail in (len(bad), min(len(bad), 2 * si.table_bytes(5) + 48), si.table_bytes(5), 16):
        rc, n, at, _ = read(bad[len(bad) - tail:], len(bad))
        if rc == si.MORE:                                       # the footer's count asks for more than this tail: give it
            need = lib().LizardGPU_seekTableBytes(n)
            assert tail < need <= len(bad), (name, tail, n)
            rc, n, at, _ = read(bad[len(bad) - need:], len(bad))
        assert rc in (si.NONE, si.DAMAGED), (name, tail, rc)
        assert at == 0, (name, "a table offset without a table")
    expect = {"the tag is another": si.NONE, "a byte behind the table": si.NONE}.get(name, si.DAMAGED)
    assert read(bad, len(bad))[0] == expect, name


def test_the_rules_cannot_refuse_a_concatenation_and_say_what_they_see():
    """Two seekable streams back to back: the second table's offsets count from its own stream's start and its last item "ends" where
    the table starts, so the rules hold with a last item that swallows everything in between (include/lizard_amd.h says so): the codec
    answers usable, and the readers' decoder is what refuses (tests/test_seek_decompress_fake_device.py, tests/test_stream_seek_gpu.py)."""
    stream, entries, end = seekable_model_stream()
    both = dict(si.lying(stream))["two seekable streams back to back"]
    rc, n, at, back = read(both, len(both))
    assert (rc, n, back) == (si.USABLE, 5, entries) and at == len(stream) + end, "the last item's region: [its offset, the second table)"


def test_need_more_tail_then_success():
    entries, end = items(1000)
    stream_bytes = end + si.table_bytes(1000)
    table = si.pack_table(entries)
    rc, n, at, _ = read(table[-16:], stream_bytes)
    assert (rc, n, at) == (si.MORE, 1000, 0)
    need = lib().LizardGPU_seekTableBytes(n)
    assert need == len(table)
    assert read(table[-(need - 1):], stream_bytes)[:2] == (si.MORE, 1000)
    assert read(table[-need:], stream_bytes) == (si.USABLE, 1000, end, entries)
    # less than a footer of a stream that could hold a table: "at least seekTableBytes(0) = 24 bytes"; of one that could not: none
    assert read(table[-15:], stream_bytes)[:2] == (si.MORE, 0)
    assert read(b"", stream_bytes)[:2] == (si.MORE, 0)
    assert read(table[-40:], 47)[0] == si.NONE


def test_every_truncation_of_a_three_item_streams_tail():
    entries, end = items(3)
    stream = bytes(end) + si.pack_table(entries)
    for k in range(len(stream) + 1):
        rc, n, at, back = read(stream[len(stream) - k:], len(stream))
        if k < 16:
            assert (rc, n) == (si.MORE, 0), k
        elif k < si.table_bytes(3):
            assert (rc, n) == (si.MORE, 3), k
        else:
            assert (rc, n, at, back) == (si.USABLE, 3, end, entries), k
    # and of the STREAM: a stream cut anywhere has no usable table (its last bytes are no footer, or the table does not tile it)
    for cut in range(1, si.table_bytes(3) + 5):
        short = stream[:len(stream) - cut]
        assert read(short, len(short))[0] in (si.NONE, si.DAMAGED), cut


def test_the_codec_as_a_stand_alone_program_under_address_sanitizer():
    """tests/seek_table_asan_main.c: round trips, every tail length and every single-bit change of a table, every buffer a heap
    allocation of exactly the bytes the codec may touch."""
    if not util.sanitizer_runtime(_dir):
        pytest.skip("no AddressSanitizer runtime: a trivial program does not build with -fsanitize=address,undefined")
    exe = os.path.join(_dir, "seek_table_asan_main")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "seek_table_asan_main.c"), os.path.join(CSRC, "lizard_seek_host.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "seek_table_asan_main: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- what every other reader of the format sees: the frames' bytes ----

@functools.lru_cache(maxsize=None)
def seekable_stream():
    """Frames made on the CPU (util.compose_frame over the oracle's blocks), two behind a tensor-header-like skippable prefix, and their
    table: (stream, the decoded bytes joined, entries)."""
    import struct
    d = util.datagen(400000, 0.5, 0.0, 77)
    parts = ((d[:70000], b""), (b"", struct.pack("<II", 0x184D2A54, 5) + b"LZT??"), (d[70000:70001], b""),
             (d[100000:100000 + 131073], struct.pack("<II", 0x184D2A54, 48) + bytes(48)))
    stream, entries = b"", []
    for data, prefix in parts:
        entries.append((len(stream), len(data), len(prefix), 0))
        stream += prefix + util.compose_frame(data, 10, 1, 1, 1, util.oracle_compress)
    return stream + write(entries), b"".join(p[0] for p in parts), entries


def frame_decoder_reads(L, stream):
    """LizardF_decompress of library L over the whole stream, call after call: the decoded bytes joined."""
    L.LizardF_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]
    L.LizardF_createDecompressionContext.restype = C.c_size_t
    L.LizardF_decompress.restype = C.c_size_t
    L.LizardF_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    L.LizardF_freeDecompressionContext.argtypes = [C.c_void_p]
    dctx = C.c_void_p()
    assert L.LizardF_createDecompressionContext(C.byref(dctx), 100) == 0
    n, cap = len(stream), 1 << 20
    src, dst = C.create_string_buffer(stream, n), C.create_string_buffer(cap)
    pos, out, r = 0, [], 0
    while pos < n:
        ds, ss = C.c_size_t(cap), C.c_size_t(n - pos)
        r = L.LizardF_decompress(dctx, dst, C.byref(ds), C.byref(src, pos), C.byref(ss), None)
        assert r < (1 << 63), "the frame decoder refused the stream at %d" % pos
        assert ss.value or ds.value
        pos += ss.value
        out.append(dst.raw[:ds.value])
    assert r == 0, "the stream ends inside a frame"
    L.LizardF_freeDecompressionContext(dctx)
    return b"".join(out)


def test_the_librarys_host_frame_decoder_steps_over_the_table():
    stream, plain, entries = seekable_stream()
    assert read(stream[-si.table_bytes(4):], len(stream)) == (si.USABLE, 4, len(stream) - si.table_bytes(4), entries)
    assert frame_decoder_reads(C.CDLL(__import__("lizard_amd._lib", fromlist=["_lib"]).LIB_PATH), stream) == plain


def test_the_references_frame_decoder_steps_over_the_table():
    ref = util.reference()
    if ref is None or not hasattr(ref, "LizardF_decompress"):
        util.need_ref("oracle/_ref/liblizard_ref_reset.so with the frame layer")
    stream, plain, _ = seekable_stream()
    assert frame_decoder_reads(ref, stream) == plain
