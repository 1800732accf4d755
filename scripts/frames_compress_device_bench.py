#!/usr/bin/env python3
"""Many buffers in device memory, one frame each: LizardGPU_compressFrames_device (one batch) against a loop of
LizardGPU_compressFrame_device over the same buffers and against the block kernels on the same bytes; same process, same input.

Input: --mib (default 1024) MiB of the tools generator's output at P50 (16 MiB pieces, consecutive seeds) in device memory, seen as
buffers of 1 MiB and as buffers of 64 KiB (views of the one tensor).  Every frame's destination is a region of its own bound inside
one output tensor, at 256-byte-aligned offsets.  Levels 10 and 30, block size id 1, with and without content checksum.  Wall clock
around calls that end in a device synchronise, GB/s of INPUT, median and min-max.
  (a) batch    LizardGPU_compressFrames_device, one call: 2 warm-ups, 5 timed repeats
  (b) loop     LizardGPU_compressFrame_device once per buffer, what a caller did before the batch entry existed: 1 warm-up, 3 timed
               repeats, over the first --loop-buffers (default 2048) buffers only — a loop over 16 384 buffers takes the better part of
               a minute per repeat; its rate is per input byte of the buffers it covered
  (c) blocks   LizardGPU_compressBlocks_device on the same bytes (blocks of 128 KiB, or of 64 KiB for the 64 KiB buffers): bound-sized
               slots and a size array, no frames: the ceiling; 2 warm-ups, 5 timed repeats
Every frame of (a) is verified by decoding it with LizardGPU_decompressFrame_device (checksum verified where there is one), and the
frames of (b) must be the same bytes.  The growth of LizardGPU_frameCompressDeviceStats over the timed repeats of (a) is recorded
([3], source bytes copied to the host, must stay 0).
The per-frame rate of the hash kernel: ONE frame of 64 MiB through the batch entry, checksum on and off.
Writes profiles/frames_compress_device.json.

    python scripts/frames_compress_device_bench.py [--mib 1024] [--loop-buffers 2048] [--out profiles/frames_compress_device.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

import util
from lizard_amd import _lib, api
import frame_decode_bench as hb

BLOCK = 128 << 10


def timed(fn, nbytes, warm, reps):
    t = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= warm:
            t.append(dt)
    rate = [nbytes / x / 1e9 for x in t]
    return {"median": round(statistics.median(rate), 3), "min": round(min(rate), 3), "max": round(max(rate), 3),
            "median_ms": round(statistics.median(t) * 1e3, 3)}


def dev_stats(L):
    s = (C.c_ulonglong * 4)()
    assert L.LizardGPU_frameCompressDeviceStats(s) == 0
    return list(s)


class Batch:
    """The arrays of one call: `count` buffers of `each` bytes of d_data, a region of the bound for every frame."""
    def __init__(self, L, d_data, each, count, p):
        self.n, self.each = count, each
        self.cap = L.LizardGPU_compressFrameBound(each, C.byref(p))
        self.pitch = (self.cap + 255) & ~255
        self.out = torch.empty(count * self.pitch, dtype=torch.uint8, device="cuda")
        self.srcs = (C.c_void_p * count)(*[d_data.data_ptr() + i * each for i in range(count)])
        self.dsts = (C.c_void_p * count)(*[self.out.data_ptr() + i * self.pitch for i in range(count)])
        self.sizes = (C.c_size_t * count)(*([each] * count))
        self.caps = (C.c_size_t * count)(*([self.cap] * count))
        self.results = (C.c_size_t * count)()

    def frame(self, i):
        return self.out[i * self.pitch:i * self.pitch + self.results[i]]


def run_batch(L, b, p, stream):
    rc = L.LizardGPU_compressFrames_device(b.n, b.dsts, b.caps, b.srcs, b.sizes, b.results, C.byref(p), stream)
    assert rc == 0, (rc, L.LizardGPU_lastError())


def run_loop(L, b, p, stream, count):
    for i in range(count):
        b.results[i] = L.LizardGPU_compressFrame_device(b.dsts[i], b.cap, b.srcs[i], b.each, C.byref(p), stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--loop-buffers", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_compress_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    L = _lib.lib()
    data = hb.gen_input(a.mib << 20)
    n = int(data.size)
    d_data = torch.from_numpy(data).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for each in (1 << 20, 64 << 10):
        count = n // each
        covered = min(count, a.loop_buffers)
        for lv, ck in [(lv, ck) for lv in (10, 30) for ck in (0, 1)]:
            p = util.frame_prefs(lv, 1, ck, 0, 1)
            row = {"buffer_bytes": each, "buffers": count, "level": lv, "checksum": bool(ck)}
            b = Batch(L, d_data, each, count, p)

            # (a) the batch entry; every frame decoded
            run_batch(L, b, p, stream)
            assert not any(L.LizardGPU_frameIsError(r) for r in b.results), L.LizardGPU_lastError()
            for i in range(count):
                back = api.decompress_frame_device(b.frame(i))
                assert torch.equal(back, d_data[i * each:(i + 1) * each]), ("a frame of the batch does not decode to its buffer", i)
            row["frame_bytes"] = int(sum(b.results))
            kept = [b.frame(i).clone() for i in range(covered)]
            s0 = dev_stats(L)
            row["batch_GBps"] = timed(lambda: run_batch(L, b, p, stream), n, 2, 5)
            row["batch_stats_delta"] = [y - x for x, y in zip(s0, dev_stats(L))]
            assert row["batch_stats_delta"][3] == 0, "source bytes were copied to the host"

            # (b) one call per buffer
            b.out.zero_()
            row["loop_buffers"] = covered
            row["loop_GBps"] = timed(lambda: run_loop(L, b, p, stream, covered), covered * each, 1, 3)
            for i in range(covered):
                assert torch.equal(b.frame(i), kept[i]), ("the single-frame entry's frame differs from the batch's", i)
            del kept

            # (c) the block kernels on the same bytes
            block = min(BLOCK, each)
            nb = n // block
            stride = (api.Lizard_compressBound(block) + 63) & ~63
            d_slots = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")

            def blocks():
                rc = L.LizardGPU_compressBlocks_device(d_data.data_ptr(), nb, block, block, d_slots.data_ptr(), stride, d_sizes.data_ptr(), lv, stream)
                assert rc == 0, L.LizardGPU_lastError()
            row["blocks_GBps"] = timed(blocks, n, 2, 5)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_slots, d_sizes, b

    # the hash kernel's pace on one frame: 64 MiB alone, checksum on and off
    one = []
    for lv in (10, 30):
        for ck in (1, 0):
            p = util.frame_prefs(lv, 1, ck, 0, 1)
            b = Batch(L, d_data, 64 << 20, 1, p)
            run_batch(L, b, p, stream)
            assert not L.LizardGPU_frameIsError(b.results[0]), L.LizardGPU_lastError()
            assert torch.equal(api.decompress_frame_device(b.frame(0)), d_data[:64 << 20]), "the 64 MiB frame does not decode to its buffer"
            r = {"buffer_bytes": 64 << 20, "buffers": 1, "level": lv, "checksum": bool(ck), "batch_GBps": timed(lambda: run_batch(L, b, p, stream), 64 << 20, 2, 5)}
            one.append(r)
            print(json.dumps(r), flush=True)
            del b
    result = {"input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "block_size_id": 1,
              "unit": "GB/s of input, wall clock around calls that end in a device synchronise",
              "repeats": {"batch": [2, 5], "loop": [1, 3], "blocks": [2, 5]}, "rows": rows, "one_frame_of_64_MiB": one}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
