#!/usr/bin/env python3
"""Many frames in device memory, each decoded into device memory: LizardGPU_decompressFrames_device (one batch) against a loop of
LizardGPU_decompressFrame_device over the same frames and against the block decoder on the same blocks; same process, same input.

Input: --mib (default 1024) MiB of the tools generator's output at P50 (16 MiB pieces, consecutive seeds) in device memory, compressed
by LizardGPU_compressFrames_device into frames of 1 MiB and into frames of 64 KiB of input (block size id 1, so 8 records or 1 record
per frame).  Every frame decodes into a region of exactly its decoded size, the regions back to back in one output tensor.  Levels 10
and 30, with and without content checksum (verified where there is one).  Wall clock around calls that end in a device synchronise,
GB/s of DECODED bytes, median and min-max.
  (a) batch    LizardGPU_decompressFrames_device, one call: 2 warm-ups, 5 timed repeats
  (b) loop     LizardGPU_decompressFrame_device once per frame, what a caller did before the batch entry existed: 1 warm-up, 3 timed
               repeats, over the first --loop-frames (default 2048) frames only; its rate is per decoded byte of the frames it covered
  (c) blocks   LizardGPU_decompressBlocks_device on the same input compressed by LizardGPU_compressBlocks_device (blocks of 128 KiB, or
               of 64 KiB for the 64 KiB frames): no frames, no checksum: the ceiling; 2 warm-ups, 5 timed repeats
The output of (a) and of (b) must be the input, byte for byte.  The growth of LizardGPU_framesDecodeDeviceStats over the timed repeats
of (a) is recorded ([2], frames handed to the single-frame entry, must stay 0).
Writes profiles/frames_decode_device.json.

    python scripts/frames_decode_device_bench.py [--mib 1024] [--loop-frames 2048] [--out profiles/frames_decode_device.json]
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
    assert L.LizardGPU_framesDecodeDeviceStats(s) == 0
    return list(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--loop-frames", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_decode_device.json"))
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
        covered = min(count, a.loop_frames)
        for lv, ck in [(lv, ck) for lv in (10, 30) for ck in (0, 1)]:
            row = {"frame_input_bytes": each, "frames": count, "level": lv, "checksum": bool(ck)}
            frames = api.compress_frames_device([d_data[i * each:(i + 1) * each] for i in range(count)], level=lv, block_size_id=1, checksum=bool(ck))
            row["frame_bytes"] = int(sum(f.numel() for f in frames))
            out = torch.empty(n, dtype=torch.uint8, device="cuda")
            srcs = (C.c_void_p * count)(*[f.data_ptr() for f in frames])
            sizes = (C.c_size_t * count)(*[int(f.numel()) for f in frames])
            dsts = (C.c_void_p * count)(*[out.data_ptr() + i * each for i in range(count)])
            caps = (C.c_size_t * count)(*([each] * count))
            results, used = (C.c_size_t * count)(), (C.c_size_t * count)()

            # (a) the batch entry
            def batch():
                rc = L.LizardGPU_decompressFrames_device(count, dsts, caps, srcs, sizes, results, used, 0, stream)
                assert rc == 0, (rc, L.LizardGPU_lastError())
            batch()
            assert all(r == each for r in results) and list(used) == list(sizes), L.LizardGPU_lastError()
            assert torch.equal(out, d_data), "the batch does not decode to the input"
            s0 = dev_stats(L)
            row["batch_GBps"] = timed(batch, n, 2, 5)
            row["batch_stats_delta"] = [y - x for x, y in zip(s0, dev_stats(L))]
            assert row["batch_stats_delta"][2] == 0, "a frame of this library was handed to the single-frame entry"

            # (b) one call per frame
            out.zero_()

            def loop():
                for i in range(covered):
                    results[i] = L.LizardGPU_decompressFrame_device(dsts[i], each, srcs[i], sizes[i], None, 0, stream)
            row["loop_frames"] = covered
            row["loop_GBps"] = timed(loop, covered * each, 1, 3)
            assert all(results[i] == each for i in range(covered)) and torch.equal(out[:covered * each], d_data[:covered * each]), "the loop does not decode to the input"
            del frames, out

            # (c) the block decoder on the same blocks
            block = min(BLOCK, each)
            nb = n // block
            stride = (api.Lizard_compressBound(block) + 63) & ~63
            d_slots = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")
            rc = L.LizardGPU_compressBlocks_device(d_data.data_ptr(), nb, block, block, d_slots.data_ptr(), stride, d_sizes.data_ptr(), lv, stream)
            assert rc == 0, L.LizardGPU_lastError()
            d_back = torch.empty(n, dtype=torch.uint8, device="cuda")
            d_outs = torch.zeros(nb, dtype=torch.int32, device="cuda")

            def blocks():
                rc = L.LizardGPU_decompressBlocks_device(d_slots.data_ptr(), stride, d_sizes.data_ptr(), nb, d_back.data_ptr(), block, d_outs.data_ptr(), stream)
                assert rc == 0, L.LizardGPU_lastError()
            row["blocks_GBps"] = timed(blocks, n, 2, 5)
            assert torch.equal(d_back, d_data), "the block decoder does not decode to the input"
            row["batch_over_loop"] = round(row["batch_GBps"]["median"] / row["loop_GBps"]["median"], 2)
            row["batch_over_blocks"] = round(row["batch_GBps"]["median"] / row["blocks_GBps"]["median"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_slots, d_sizes, d_back, d_outs
    result = {"input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "block_size_id": 1,
              "unit": "GB/s of decoded bytes, wall clock around calls that end in a device synchronise",
              "repeats": {"batch": [2, 5], "loop": [1, 3], "blocks": [2, 5]}, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
