#!/usr/bin/env python3
"""Whole-frame compression of data that lies in device memory: LizardGPU_compressFrame_device against its host-memory twin and
against the block kernels on the same blocks, same process, same input.

Input: --mib (default 1024) MiB of the tools generator's output at P50 (16 MiB pieces, consecutive seeds); one frame of
independent blocks per configuration: levels 10 and 30, block size ids 2 (256 KiB) and 4 (4 MiB), with and without content
checksum.  Per configuration, 2 warm-ups and 5 timed repeats of each path, wall clock around a call that ends in a device
synchronise, GB/s of INPUT, median and min-max.  Every path's frame is verified once by decoding it (the device entry's with
LizardGPU_decompressFrame_device, checksum verified; the twin's frame must be the same bytes).
  (a) device      LizardGPU_compressFrame_device: input and frame in device memory
  (b) host_twin   LizardGPU_compressFrame: the same bytes and the frame in pinned host memory
  (c) blocks      LizardGPU_compressBlocks_device on the same blocks: bound-sized slots and a size array, no frame: the ceiling
The counters of LizardGPU_frameCompressDeviceStats over the timed repeats of (a) are recorded.  Writes
profiles/frame_compress_device.json.

    python scripts/frame_compress_device_bench.py [--mib 1024] [--out profiles/frame_compress_device.json]
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
import numpy as np
import torch

import util
from lizard_amd import _lib, api
import frame_decode_bench as hb

WARM, REPS = 2, 5


def timed(fn, nbytes):
    t = []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= WARM:
            t.append(dt)
    rate = [nbytes / x / 1e9 for x in t]
    return {"median": round(statistics.median(rate), 3), "min": round(min(rate), 3), "max": round(max(rate), 3),
            "median_ms": round(statistics.median(t) * 1e3, 3)}


def dev_stats(L):
    s = (C.c_ulonglong * 4)()
    assert L.LizardGPU_frameCompressDeviceStats(s) == 0
    return list(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_compress_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    L = _lib.lib()
    hb.host_api(L)
    data = hb.gen_input(a.mib << 20)
    n = int(data.size)
    d_data = torch.from_numpy(data).cuda()
    h_data = torch.from_numpy(data).pin_memory()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for lv, bsid, ck in [(lv, bsid, ck) for lv in (10, 30) for bsid in (2, 4) for ck in (0, 1)]:
        block = util.FRAME_BLOCK_SIZES[bsid]
        p = util.frame_prefs(lv, bsid, ck, 0, 1)
        cap = L.LizardGPU_compressFrameBound(n, C.byref(p))
        d_frame = torch.empty(cap, dtype=torch.uint8, device="cuda")
        h_frame = torch.empty(cap, dtype=torch.uint8).pin_memory()
        row = {"level": lv, "block_size_id": bsid, "block_bytes": block, "checksum": bool(ck)}
        size = {}

        # (a) the device entry
        def device():
            r = L.LizardGPU_compressFrame_device(d_frame.data_ptr(), cap, d_data.data_ptr(), n, C.byref(p), stream)
            assert not L.LizardGPU_frameIsError(r), (L.LizardF_getErrorName(r), L.LizardGPU_lastError())
            size["device"] = r
        device()
        back = api.decompress_frame_device(d_frame[:size["device"]])
        assert torch.equal(back, d_data), "the device entry's frame does not decode to the input"
        del back
        s0 = dev_stats(L)
        row["device_GBps"] = timed(device, n)
        row["device_stats_delta"] = [y - x for x, y in zip(s0, dev_stats(L))]
        row["frame_bytes"] = int(size["device"])

        # (b) the host twin, pinned memory on both sides
        def host_twin():
            r = L.LizardGPU_compressFrame(h_frame.data_ptr(), cap, h_data.data_ptr(), n, C.byref(p))
            assert not L.LizardGPU_frameIsError(r), (L.LizardF_getErrorName(r), L.LizardGPU_lastError())
            size["twin"] = r
        host_twin()
        assert size["twin"] == size["device"] and torch.equal(h_frame[:size["twin"]], d_frame[:size["device"]].cpu()), "the twin's frame differs"
        row["host_twin_GBps"] = timed(host_twin, n)

        # (c) the block kernels on the same blocks
        nb = (n + block - 1) // block
        stride = (api.Lizard_compressBound(block) + 63) & ~63
        d_slots = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")

        def blocks():
            rc = L.LizardGPU_compressBlocks_device(d_data.data_ptr(), nb, block, n - (nb - 1) * block, d_slots.data_ptr(), stride, d_sizes.data_ptr(), lv, stream)
            assert rc == 0, L.LizardGPU_lastError()
        blocks()
        torch.cuda.synchronize()
        dec, out_sizes = api.decompress_blocks_device(d_slots, d_sizes, stride, block)
        torch.cuda.synchronize()
        assert torch.equal(dec[:n], d_data) and int(out_sizes.sum().item()) == n, "the blocks do not decode to the input"
        del dec
        row["blocks_GBps"] = timed(blocks, n)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_slots, d_frame, h_frame
    result = {"input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "repeats": REPS, "warmups": WARM,
              "unit": "GB/s of input, wall clock around a call that ends in a device synchronise", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
