"""LizardGPU_frameIndex / LizardGPU_decompressFrameBound: the host walk LizardGPU_decompressFrame works from (no device needed).

The record table is compared with a plain Python walk of the frame format, the refusals with what the library's own streaming
decoder LizardF_decompress answers when it is fed the same bytes in one call.  That decoder cannot refuse a frame that merely
ends early — it returns a hint and waits for more input — so for those the one-call contract of include/lizard_amd.h (Part 3b) is
checked: frameHeader_incomplete while the header is not complete (what LizardF_getFrameInfo answers for the same bytes), GENERIC
behind it."""
import ctypes as C
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util

E_GENERIC, E_HEADER_INCOMPLETE, E_FRAMETYPE = 1, 12, 13
BS = util.FRAME_BLOCK_SIZES


def lib():
    from lizard_amd import _lib
    L = _lib.lib()
    L.LizardF_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]; L.LizardF_createDecompressionContext.restype = C.c_size_t
    L.LizardF_freeDecompressionContext.argtypes = [C.c_void_p]; L.LizardF_freeDecompressionContext.restype = C.c_size_t
    L.LizardF_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.LizardF_decompress.restype = C.c_size_t
    L.LizardF_getFrameInfo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]; L.LizardF_getFrameInfo.restype = C.c_size_t
    L.LizardF_isError.argtypes = [C.c_size_t]; L.LizardF_isError.restype = C.c_uint
    return L


def err_of(code):
    """0 for a size / hint, else the positive LizardF_ERROR_* number of a size_t result."""
    return (1 << 64) - code if lib().LizardF_isError(code) else 0


def host_one_call(frame, cap):
    """LizardF_decompress fed the whole input in one call: (error number or 0, hint, consumed, bytes)."""
    L = lib()
    d = C.c_void_p()
    assert L.LizardF_createDecompressionContext(C.byref(d), 100) == 0
    dst = C.create_string_buffer(max(cap, 1))
    src = C.create_string_buffer(bytes(frame), max(len(frame), 1))
    dn, sn = C.c_size_t(cap), C.c_size_t(len(frame))
    r = L.LizardF_decompress(d, dst, C.byref(dn), src, C.byref(sn), None)
    L.LizardF_freeDecompressionContext(d)
    e = err_of(r)
    return e, (0 if e else r), sn.value, dst.raw[:dn.value]


def host_frame_info_error(frame):
    L = lib()
    d = C.c_void_p()
    assert L.LizardF_createDecompressionContext(C.byref(d), 100) == 0
    info = util.FrameInfo()
    src = C.create_string_buffer(bytes(frame), max(len(frame), 1))
    sn = C.c_size_t(len(frame))
    r = L.LizardF_getFrameInfo(d, C.byref(info), src, C.byref(sn))
    L.LizardF_freeDecompressionContext(d)
    return err_of(r)


def index(frame, max_records=None):
    """(rc, info, offsets, words, nRecords, frameBytes) of LizardGPU_frameIndex."""
    L = lib()
    src = C.create_string_buffer(bytes(frame), max(len(frame), 1))
    info = util.FrameInfo()
    n, fb = C.c_size_t(0), C.c_size_t(0)
    rc = L.LizardGPU_frameIndex(src, len(frame), C.byref(info), None, None, 0, C.byref(n), C.byref(fb))
    if rc:
        return rc, info, [], [], n.value, fb.value
    m = n.value if max_records is None else max_records
    offs, words = (C.c_uint64 * max(m, 1))(), (C.c_uint32 * max(m, 1))()
    rc = L.LizardGPU_frameIndex(src, len(frame), C.byref(info), offs, words, m, C.byref(n), C.byref(fb))
    return rc, info, list(offs)[:min(m, n.value)], list(words)[:min(m, n.value)], n.value, fb.value


def bound(frame):
    src = C.create_string_buffer(bytes(frame), max(len(frame), 1))
    return lib().LizardGPU_decompressFrameBound(src, len(frame))


def python_walk(frame):
    """The frame format, plainly: (offsets, words, frameBytes, sum bound)."""
    assert struct.unpack_from("<I", frame, 0)[0] == 0x184D2206
    flg, bd = frame[4], frame[5]
    pos = 15 if flg & 8 else 7
    block = BS[(bd >> 4) & 7]
    offs, words, total = [], [], 0
    while True:
        word = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
        size = word & 0x7FFFFFFF
        if size == 0:
            break
        offs.append(pos); words.append(word)
        total += size if word >> 31 else block
        pos += size
    if flg & 4:
        pos += 4
    return offs, words, pos, total


def frames_of_cases():
    data = dict(util.corpus())
    out = []
    for name, case, level, bsid, checksum, csize in util.FRAME_CASES:
        out.append((name, util.compose_frame(data[case], level, bsid, checksum, csize, util.oracle_compress), data[case], bool(csize)))
    return out


def check_against_walk(name, frame, plain, has_size):
    rc, info, offs, words, n, fb = index(frame)
    woffs, wwords, wfb, wsum = python_walk(frame)
    assert rc == 0, name
    assert (n, offs, words, fb) == (len(woffs), woffs, wwords, wfb), name
    assert info.contentChecksumFlag == (frame[4] >> 2) & 1 and info.blockMode == (frame[4] >> 5) & 1 and info.blockSizeID == frame[5] >> 4
    b = bound(frame)
    assert not err_of(b), name
    if has_size and len(plain):
        assert info.contentSize == len(plain) and b == len(plain), name
    else:
        assert b == wsum >= len(plain), name
    # a short table is filled as far as it goes and still reports the frame's count
    if n > 1:
        rc2, _, o2, w2, n2, fb2 = index(frame, 1)
        assert (rc2, o2, w2, n2, fb2) == (0, woffs[:1], wwords[:1], n, fb)
    # the same frame followed by other bytes: the index ends where the frame ends
    rc3, _, o3, _, n3, fb3 = index(frame + b"\x04\x22\x4d\x18tail")
    assert (rc3, o3, n3, fb3) == (0, woffs, n, fb)
    e, hint, used, got = host_one_call(frame, len(plain) + 16)
    assert (e, hint, used, got) == (0, 0, fb, plain), name


def test_index_matches_a_plain_walk():
    for name, frame, plain, has_size in frames_of_cases():
        check_against_walk(name, frame, plain, has_size)


def test_index_of_reference_made_frames():
    if util.reference() is None:
        util.need_ref("oracle/_ref/liblizard_ref_reset.so")
    data = util.datagen(3 * 131072 + 777, 0.5, 0.0, 41)
    for mode in (0, 1):
        for level, bsid, checksum, csize in ((10, 1, 1, 0), (17, 1, 0, 1), (30, 2, 1, 1), (41, 1, 0, 0)):
            p = util.frame_prefs(level, bsid, checksum, len(data) if csize else 0, mode)
            check_against_walk("ref mode %d L%d" % (mode, level), util.reference_frame(data, p), data, bool(csize))


def test_skippable_frame():
    f = struct.pack("<II", 0x184D2A53, 5) + b"hello"
    rc, info, offs, words, n, fb = index(f + b"more")
    assert (rc, info.frameType, info.contentSize, n, fb) == (0, 1, 5, 0, 13)
    assert bound(f) == 0
    assert index(f[:7])[0] == -E_HEADER_INCOMPLETE and index(f[:12])[0] == -E_GENERIC


def small_frame(csize):
    data = util.datagen(700, 0.5, 0.0, 9) + bytes(range(256)) * 2
    return util.compose_frame(data, 10, 1, 1, csize, util.oracle_compress), data


def test_header_refusals_match_the_host_decoder():
    import xxhash
    seen = set()
    for csize in (0, 1):
        frame, data = small_frame(csize)
        hsize = 15 if csize else 7

        def with_header(flg=None, bd=None, fix=True, magic=None):
            h = bytearray(frame[:hsize])
            if flg is not None:
                h[4] = flg
            if bd is not None:
                h[5] = bd
            if fix:
                h[hsize - 1] = (xxhash.xxh32(bytes(h[4:hsize - 1]), seed=0).intdigest() >> 8) & 255
            if magic is not None:
                h[0:4] = struct.pack("<I", magic)
            return bytes(h) + frame[hsize:]
        flg, bd = frame[4], frame[5]
        cases = [with_header(flg=(flg & 0x3F) | v << 6) for v in (0, 2, 3)]             # version
        cases += [with_header(flg=flg | 0x10), with_header(flg=flg | 1), with_header(flg=flg | 2)]   # block checksum, reserved
        cases += [with_header(bd=bd | 0x80), with_header(bd=bd & 0x0F), with_header(bd=bd | 1), with_header(bd=bd | 8)]
        cases += [with_header(bd=(bd & 0x8F) | 7 << 4, fix=False)]                            # header checksum
        cases += [frame[:hsize - 1] + bytes([frame[hsize - 1] ^ 0x40]) + frame[hsize:]]
        cases += [with_header(magic=0x184D2207), with_header(magic=0), with_header(magic=0x184D2A60)]
        for bad in cases:
            e, hint, used, got = host_one_call(bad, len(data) + 16)
            assert e, "the host decoder accepts a header this test meant to break"
            assert index(bad)[0] == -e
            assert err_of(bound(bad)) == e
            seen.add(e)
    assert seen >= {2, 6, 7, 8, 13, 17}, seen          # maxBlockSize, version, block checksum, reserved, frame type, header checksum


def test_every_truncation_point():
    for csize in (0, 1):
        frame, data = small_frame(csize)
        hsize = 15 if csize else 7
        for cut in range(len(frame) + 1):
            part = frame[:cut]
            rc = index(part)[0]
            e, hint, used, got = host_one_call(part, len(data) + 16)
            if cut == len(frame):
                assert (rc, e, hint) == (0, 0, 0)
                continue
            assert e == 0 and (hint > 0 or cut == 0), "the host decoder refuses a prefix of a valid frame"
            if cut < hsize:
                assert rc == -E_HEADER_INCOMPLETE, cut
                if cut:
                    assert host_frame_info_error(part) == E_HEADER_INCOMPLETE, cut
            else:
                assert rc == -E_GENERIC, cut
            assert err_of(bound(part)) == -rc


def test_record_words_the_host_decoder_refuses():
    frame, data = small_frame(0)
    big = bytearray(frame)
    big[7:11] = struct.pack("<I", BS[1] + 1)                       # larger than the frame's block size
    e, hint, used, got = host_one_call(bytes(big) + bytes(BS[1]), len(data) + 16)
    assert e == E_GENERIC and index(bytes(big) + bytes(BS[1]))[0] == -E_GENERIC
    early = bytearray(frame)
    early[7:11] = struct.pack("<I", 0)                             # an end mark in place of the first record: a shorter, valid chain
    rc, info, offs, words, n, fb = index(bytes(early))
    assert (rc, n, fb) == (0, 0, 7 + 4 + 4)
