#!/usr/bin/env python3
"""Whole-frame decompression: LizardGPU_decompressFrame against the host LizardF_decompress (whole frame in one call), same
process, same frame.

Input: --mib (default 1024) MiB of the tools generator's output at P50, generated in 16 MiB pieces with consecutive seeds.
Configurations: levels 10 and 30, block size ids 2 (256 KiB) and 4 (4 MiB), independent and library-made linked frames, with
and without content checksum; plus one frame made by the compiled reference in linked mode when oracle/_ref is present (64 MiB
of the input: the reference compresses on one thread).  Per configuration: 2 warm-ups, 5 timed repeats of each decoder,
wall-clock GB/s of OUTPUT, median and min-max; the output is compared byte for byte with the input every time; the decode
counters (LizardGPU_frameDecodeStats) of the timed repeats are printed.  Writes profiles/frame_decode_<commit>.json.

    python scripts/frame_decode_bench.py [--mib 1024] [--out profiles/frame_decode_<commit>.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import util
from lizard_amd import _lib
from tools import datagen


def host_api(L):
    L.LizardF_createDecompressionContext.argtypes = [C.c_void_p, C.c_uint]; L.LizardF_createDecompressionContext.restype = C.c_size_t
    L.LizardF_freeDecompressionContext.argtypes = [C.c_void_p]; L.LizardF_freeDecompressionContext.restype = C.c_size_t
    L.LizardF_decompress.argtypes = [C.c_void_p] * 6; L.LizardF_decompress.restype = C.c_size_t
    L.LizardF_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]; L.LizardF_compressFrame.restype = C.c_size_t
    L.LizardF_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]; L.LizardF_compressFrameBound.restype = C.c_size_t


def gen_input(n):
    buf = np.empty(n, dtype=np.uint8)
    piece = 16 << 20
    for i, off in enumerate(range(0, n, piece)):
        m = min(piece, n - off)
        datagen.datagen_host(C.c_void_p(buf.ctypes.data + off), m, 0.5, 0.0, 1000 + i)
    return buf


def make_frame(L, data, level, bsid, checksum, mode):
    p = util.frame_prefs(level, bsid, checksum, data.size, mode)
    cap = L.LizardF_compressFrameBound(data.size, C.byref(p))
    dst = np.empty(cap, dtype=np.uint8)
    n = L.LizardF_compressFrame(dst.ctypes.data, cap, data.ctypes.data, data.size, C.byref(p))
    assert not L.LizardGPU_frameIsError(n), L.LizardF_getErrorName(n)
    return dst[:n].copy()


def gpu_decode(L, frame, out):
    used = C.c_size_t(0)
    n = L.LizardGPU_decompressFrame(out.ctypes.data, out.size, frame.ctypes.data, frame.size, C.byref(used))
    assert not L.LizardGPU_frameIsError(n), (L.LizardF_getErrorName(n), L.LizardGPU_lastError())
    assert used.value == frame.size
    return n


def host_decode(L, frame, out):
    d = C.c_void_p()
    assert L.LizardF_createDecompressionContext(C.byref(d), 100) == 0
    dn, sn = C.c_size_t(out.size), C.c_size_t(frame.size)
    r = L.LizardF_decompress(d, out.ctypes.data, C.byref(dn), frame.ctypes.data, C.byref(sn), None)
    L.LizardF_freeDecompressionContext(d)
    assert r == 0 and sn.value == frame.size, r
    return dn.value


def stats(L):
    s = (C.c_ulonglong * 4)()
    L.LizardGPU_frameDecodeStats(s)
    return list(s)


def measure(L, fn, frame, data, out, warm=2, reps=5):
    t = []
    for i in range(warm + reps):
        out[:] = 0
        t0 = time.perf_counter()
        n = fn(L, frame, out)
        dt = time.perf_counter() - t0
        assert n == data.size and np.array_equal(out[:n], data), "decoded bytes differ from the input"
        if i >= warm:
            t.append(data.size / dt / 1e9)
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    host_api(L)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "worktree"
    data = gen_input(a.mib << 20)
    out = np.empty(data.size, dtype=np.uint8)
    rows = []
    configs = [(lv, bsid, mode, ck) for lv in (10, 30) for bsid in (2, 4) for mode in (1, 0) for ck in (0, 1)]
    for lv, bsid, mode, ck in configs:
        frame = make_frame(L, data, lv, bsid, ck, mode)
        s0 = stats(L)
        g = measure(L, gpu_decode, frame, data, out)
        s1 = stats(L)
        h = measure(L, host_decode, frame, data, out)
        row = {"origin": "library", "level": lv, "block_size_id": bsid, "mode": "independent" if mode else "linked", "checksum": bool(ck),
               "frame_bytes": int(frame.size), "gpu_GBps": g, "host_GBps": h, "gpu_slowest_beats_host_fastest": g["min"] > h["max"],
               "stats_delta": [b - x for x, b in zip(s0, s1)]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if util.reference() is not None:
        small = data[:min(data.size, 64 << 20)]
        frame = np.frombuffer(util.reference_frame(small.tobytes(), util.frame_prefs(10, 2, 1, small.size, 0)), dtype=np.uint8).copy()
        o = out[:small.size]
        s0 = stats(L)
        g = measure(L, gpu_decode, frame, small, o)
        s1 = stats(L)
        h = measure(L, host_decode, frame, small, o)
        row = {"origin": "reference", "level": 10, "block_size_id": 2, "mode": "linked", "checksum": True, "frame_bytes": int(frame.size),
               "input_MiB": small.size >> 20, "gpu_GBps": g, "host_GBps": h, "stats_delta": [b - x for x, b in zip(s0, s1)]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"commit": commit, "input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "repeats": 5, "warmups": 2,
              "unit": "GB/s of decoded output, wall clock", "rows": rows}
    path = a.out or os.path.join(ROOT, "profiles", "frame_decode_%s.json" % commit)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
