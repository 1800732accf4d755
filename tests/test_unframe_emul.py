"""The record body of lz_unframe_kernel (lizard_amd/csrc/unframe_kernels.h) on the CPU SIMT emulator: raw records at every source
misalignment, the history-aware return of the block decoder (LZD_NEED_HISTORY exactly where a block of a linked frame reaches in
front of its own start), and the unchanged entry beside it."""
import ctypes as C
import functools
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import test_gpu_decoder_differential as dd

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
NEED_HISTORY, ERR = 0xFFFFFFFE, 0xFFFFFFFF
SEEDS = (1, 0x9E3779B9)
CANARY = 0xC3


@functools.lru_cache(maxsize=None)
def unframe_lib():
    """tests/emul/libunframe_emul.so from simt.cpp + unframe_api.cpp, the way tests/emul/build.py builds libemul.so."""
    out = os.path.join(EMUL, "libunframe_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "unframe_api.cpp")]
    csrc = os.path.join(util.ROOT, "lizard_amd", "csrc")
    deps = srcs + [os.path.join(EMUL, "lz_wave.h")] + [os.path.join(csrc, f) for f in ("unframe_kernels.h", "lz_unpack.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_unframe_record.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint]
    L.emul_unframe_record.restype = C.c_uint
    return L


def run_record(payload, word, cap, seed, misalign=0):
    """One record with canaries on both sides of the payload and of the slot: (result, slot bytes up to the result)."""
    g = 64
    src = (C.c_ubyte * (len(payload) + 2 * g + 16))()
    C.memset(src, 0x5A, len(src))
    C.memmove(C.addressof(src) + g + misalign, payload, len(payload))
    out = (C.c_ubyte * (cap + 2 * g))()
    C.memset(out, CANARY, len(out))
    r = unframe_lib().emul_unframe_record(C.addressof(src) + g + misalign, len(payload), word, C.addressof(out) + g, cap, seed)
    raw = bytes(out)
    assert raw[:g] == bytes([CANARY]) * g and raw[g + cap:] == bytes([CANARY]) * g, "the record body wrote outside its slot"
    if r >= NEED_HISTORY:
        return r, b""
    assert r <= cap
    assert raw[g + r:g + cap] == bytes([CANARY]) * (cap - r), "bytes behind the decoded size were written"
    return r, raw[g:g + r]


def both_seeds(payload, word, cap, misalign=0):
    a = run_record(payload, word, cap, SEEDS[0], misalign)
    assert a == run_record(payload, word, cap, SEEDS[1], misalign), "two lane schedules disagree"
    return a


def test_raw_records_at_every_misalignment():
    import random
    rnd = random.Random(5)
    for n in (1, 15, 16, 17, 4097):
        data = rnd.randbytes(n)
        for mis in range(16):
            assert both_seeds(data, n | 0x80000000, 8192, mis) == (n, data)
        assert both_seeds(data, n | 0x80000000, n)[1] == data                      # the slot exactly as large as the record
        assert both_seeds(data, n | 0x80000000, n - 1)[0] == ERR if n > 1 else True   # a record larger than its slot is refused
    assert both_seeds(b"x", 0x80000000, 64)[0] == ERR and both_seeds(b"x", 0, 64)[0] == ERR   # size 0 never reaches a decoder


def frame_records(frame):
    flg, bd = frame[4], frame[5]
    pos = 15 if flg & 8 else 7
    out = []
    while True:
        word = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
        if word & 0x7FFFFFFF == 0:
            return out, util.FRAME_BLOCK_SIZES[(bd >> 4) & 7]
        out.append((word, frame[pos:pos + (word & 0x7FFFFFFF)]))
        pos += word & 0x7FFFFFFF


def test_reference_linked_frames_need_history_exactly_where_a_standalone_decode_fails():
    ref = dd.need_reference()
    seen = {"hist": 0, "ok": 0}
    inputs = [util.datagen(5 * 131072 + 999, 0.5, 0.0, 21), (b"the quick brown fox jumps over the lazy dog. " * 20000)[:4 * 131072 + 5]]
    for data in inputs:
        for level in (10, 17, 30, 41):
            for mode in (0, 1):
                frame = util.reference_frame(data, util.frame_prefs(level, 1, 0, 0, mode))
                records, block = frame_records(frame)
                pos = 0
                for word, payload in records:
                    plain = data[pos:pos + block]
                    pos += len(plain)
                    if word >> 31:
                        assert both_seeds(payload, word, block) == (len(plain), plain)
                        continue
                    alone = dd.ref_decode(payload, block)
                    r, got = both_seeds(payload, word, block)
                    if alone[0] == dd.ERR:
                        assert mode == 0 and r == NEED_HISTORY, "a valid block the reference cannot decode alone must need its history"
                        seen["hist"] += 1
                    else:
                        assert (r, got) == (len(plain), plain) and alone[1] == plain
                        seen["ok"] += 1
                assert pos == len(data)
    assert seen["hist"] > 20 and seen["ok"] > 20, seen


def test_offset_edges_through_both_entries():
    emu = util.emulator()
    emu.emul_decompress_block.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint]
    emu.emul_decompress_block.restype = C.c_int
    kinds = {"ok": 0, "hist": 0, "zero": 0}
    for name, block, plain, _ in dd.offset_edge_vectors():
        r, got = both_seeds(block, len(block), 4096)
        out = C.create_string_buffer(4096)
        old = emu.emul_decompress_block(block, len(block), out, 4096, 1)
        if plain is not None:
            assert (r, got) == (len(plain), plain) and old == len(plain) and out.raw[:old] == plain, name
            kinds["ok"] += 1
        elif name.endswith("offset 0"):
            assert r == ERR and old == -1, name
            kinds["zero"] += 1
        else:
            assert r == NEED_HISTORY and old == -1, name                             # off = op + 1
            kinds["hist"] += 1
    assert min(kinds.values()) == 18, kinds


def test_hand_built_vectors_decode_the_same_through_the_new_body():
    for name, block, plain, _ in dd.match_vectors():
        cap = len(plain)
        assert both_seeds(block, len(block), cap) == (len(plain), plain), name
        assert run_record(block, len(block), cap - 1, 1)[0] == ERR, name             # one byte short: refused, not "needs history"
