"""CPU: the body of lz_stream_seektable_kernel (lz_stream_seektable_item, lizard_amd/csrc/lz_stream_pack.h) on the SIMT emulator, launched
the way lz_stream_seektable_launch launches it, against the host codec (LizardGPU_seekTableWrite): n = 1, 63, 64, 65, 1 000 items,
the table starting at every byte address mod 4, items without blocks (their offsets are the finish kernel's, which the test supplies),
and with the overflow flag set or a total above the capacity NOTHING is written: the 0x5A canaries around and under the table hold."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import seek_inputs as si
from test_seek_table import Entry as SeekEntry, lib as product

EMUL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
SEEDS = (1, 0x9E3779B9)
GUARD = 64


class FramesEntry(C.Structure):                                # LzFramesEntry (lizard_gpu_ctx.h)
    _fields_ = [("dst", C.c_uint64), ("limit", C.c_uint64), ("cursor", C.c_uint64), ("src", C.c_uint64), ("srcSize", C.c_uint64),
                ("overflow", C.c_uint32), ("rawRecords", C.c_uint32), ("blockSize", C.c_uint32), ("nBlocks", C.c_uint32), ("hash", C.c_uint32),
                ("headerBytes", C.c_uint32), ("flags", C.c_uint32), ("header", C.c_uint8 * 20)]


class StreamEntry(C.Structure):                                # LzStreamEntry
    _fields_ = [("fixed", C.c_uint64), ("before", C.c_uint64), ("prefixOff", C.c_uint64), ("prefixBytes", C.c_uint64), ("firstBlock", C.c_uint32),
                ("lastBlock", C.c_uint32), ("nextSelf", C.c_uint32), ("nextAfter", C.c_uint32), ("tailBytes", C.c_uint32), ("reserved", C.c_uint32)]


class StreamState(C.Structure):                                # LzStreamState
    _fields_ = [("carry", C.c_uint64), ("overflow", C.c_uint32), ("rawRecords", C.c_uint32)]


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emul/libseektable_emul.so from simt.cpp + seektable_api.cpp, the way test_planes_xor_emul.py builds its library (plus the
    HIP runtime's headers, which lizard_gpu_ctx.h's tables need)."""
    out = os.path.join(EMUL, "libseektable_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "seektable_api.cpp")]
    csrc = os.path.join(util.ROOT, "lizard_amd", "csrc")
    deps = srcs + [os.path.join(EMUL, "lz_wave.h"), os.path.join(csrc, "lz_stream_pack.h"), os.path.join(csrc, "lizard_gpu_ctx.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                               "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = C.CDLL(out)
    L.emul_seektable.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_ulonglong, C.c_ulonglong, C.c_uint]
    L.emul_seektable.restype = C.c_uint
    return L


def test_the_tables_have_the_host_files_layout():
    L = lib()
    assert L.emul_seektable_frames_entry_bytes() == C.sizeof(FramesEntry) == 88
    assert L.emul_seektable_stream_entry_bytes() == C.sizeof(StreamEntry) == 56
    assert L.emul_seektable_state_bytes() == C.sizeof(StreamState) == 16


def items(n, rng):
    """n items as the finish kernel leaves them: (offset, source size, prefix bytes); about a quarter have no blocks (size 0) and a
    third no prefix.  Returns them and where the last one ends."""
    out, pos = [], 0
    for i in range(n):
        size = 0 if rng.integers(4) == 0 else int(rng.integers(1, 1 << 33))
        pre = 0 if rng.integers(3) == 0 else int(rng.integers(8, 121))
        out.append((pos, size, pre))
        pos += pre + 19 + (int(rng.integers(1, 5000)) if size else 0)
    return out, pos


def run(n, skew, seed, overflow=0, short=0):
    """One launch for n items whose table starts at an address that is `skew` mod 4.  Returns (the buffer with GUARD bytes of 0x5A on
    both sides, where the stream starts in it, the items, the stream's size)."""
    L = lib()
    rng = np.random.default_rng(1000 * n + skew)
    its, end = items(n, rng)
    end += (skew - end) % 4                                     # (the last frame's bytes: whatever makes the table start there)
    total = end + si.table_bytes(n)
    raw = np.full(GUARD + total + GUARD + 8, 0x5A, dtype=np.uint8)
    at = GUARD + (-(raw.ctypes.data + GUARD)) % 4               # the stream's first byte is 4-byte aligned: the table's address is skew mod 4
    assert (raw.ctypes.data + at + end) % 4 == skew
    frames, entries, offsets = (FramesEntry * n)(), (StreamEntry * n)(), (C.c_uint64 * (n + 1))()
    for i, (off, size, pre) in enumerate(its):
        frames[i].dst, frames[i].limit, frames[i].srcSize = raw.ctypes.data + at, total, size
        entries[i].prefixBytes = pre
        offsets[i] = off
    offsets[n] = total
    fixed = 12345 + si.table_bytes(n)
    state = StreamState(total - fixed, overflow, 0)
    threads = L.emul_seektable(frames, entries, C.byref(state), offsets, n, fixed, total - short, seed)
    assert threads == (n // 256 + 1) * 256
    return raw, at, its, total


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1000))
def test_the_table_equals_the_host_codecs(n, seed):
    P = product()
    for skew in range(4):
        raw, at, its, total = run(n, skew, seed)
        want = C.create_string_buffer(si.table_bytes(n))
        arr = (SeekEntry * n)(*[SeekEntry(off, size, pre, 0) for off, size, pre in its])
        assert P.LizardGPU_seekTableWrite(want, len(want), arr, n) == si.table_bytes(n)
        start = at + total - si.table_bytes(n)
        assert raw[start:at + total].tobytes() == want.raw == si.pack_table(its), (n, skew)
        assert (raw[:start] == 0x5A).all() and (raw[at + total:] == 0x5A).all(), (n, skew, "a byte outside the table was written")
        # and the host codec finds it usable, with these entries
        n_out, t_out = C.c_size_t(0), C.c_uint64(0)
        back = (SeekEntry * n)()
        assert P.LizardGPU_seekTableRead(raw[start:at + total].tobytes(), si.table_bytes(n), total, back, n, C.byref(n_out), C.byref(t_out)) == si.USABLE
        assert (n_out.value, t_out.value) == (n, total - si.table_bytes(n))
        assert [(e.offset, e.decodedBytes, e.prefixBytes, e.flags) for e in back] == [i + (0,) for i in its]


@pytest.mark.parametrize("n", (1, 65, 1000))
def test_after_an_overflow_nothing_is_written(n):
    for skew, overflow, short in ((0, 1, 0), (3, 0, 1), (1, 1, 1), (2, 0, si.table_bytes(n))):
        raw, at, its, total = run(n, skew, SEEDS[0], overflow, short)
        assert (raw == 0x5A).all(), (n, skew, overflow, short)
