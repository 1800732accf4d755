#!/usr/bin/env python3
"""Whole-frame decompression of a frame that lies in device memory: LizardGPU_decompressFrame_device against its host-memory twin
and against the block decoder on the same blocks, same process, same frame.

Input: --mib (default 1024) MiB of the tools generator's output at P50 (16 MiB pieces, consecutive seeds), one frame of
independent blocks per configuration: levels 10 and 30, block size ids 2 (256 KiB) and 4 (4 MiB), with and without content
checksum.  Per configuration, 2 warm-ups and 5 timed repeats of each path, wall clock around a call that ends in a device
synchronise, GB/s of OUTPUT, median and min-max; the decoded bytes of every path are compared with the input once.
  (a) host_twin     LizardGPU_decompressFrame: frame and output in pageable host memory
  (b) device        LizardGPU_decompressFrame_device: frame and output in device memory; for a frame with a checksum also
      device_skip   the same with LIZARDGPU_FRAME_SKIP_CHECKSUM
  (c) blocks        LizardGPU_decompressBlocks_device on the frame's blocks laid out in slots beforehand: the ceiling
  (d) walk          LizardGPU_frameIndex_device without tables: the walk alone, in ms and ns per record
The counters of LizardGPU_frameDecodeDeviceStats over the timed repeats of (b) are recorded.  Writes
profiles/frame_decode_device.json.

    python scripts/frame_decode_device_bench.py [--mib 1024] [--out profiles/frame_decode_device.json]
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
from lizard_amd import _lib
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
    assert L.LizardGPU_frameDecodeDeviceStats(s) == 0
    return list(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_decode_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    L = _lib.lib()
    hb.host_api(L)
    data = hb.gen_input(a.mib << 20)
    d_data = torch.from_numpy(data).cuda()
    out = np.empty(data.size, dtype=np.uint8)
    d_out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for lv, bsid, ck in [(lv, bsid, ck) for lv in (10, 30) for bsid in (2, 4) for ck in (0, 1)]:
        frame = hb.make_frame(L, data, lv, bsid, ck, 1)
        d_frame = torch.from_numpy(frame).cuda()
        block = util.FRAME_BLOCK_SIZES[bsid]
        row = {"level": lv, "block_size_id": bsid, "block_bytes": block, "checksum": bool(ck), "frame_bytes": int(frame.size)}

        # (a) the host twin
        out[:] = 0
        assert hb.gpu_decode(L, frame, out) == data.size and np.array_equal(out, data)
        row["host_twin_GBps"] = timed(lambda: hb.gpu_decode(L, frame, out), data.size)

        # (b) the device entry
        def device(flags):
            used = C.c_size_t(0)
            n = L.LizardGPU_decompressFrame_device(d_out.data_ptr(), d_out.numel(), d_frame.data_ptr(), d_frame.numel(), C.byref(used), flags, stream)
            assert not L.LizardGPU_frameIsError(n), (L.LizardF_getErrorName(n), L.LizardGPU_lastError())
            assert n == data.size and used.value == frame.size
        for name, flags in [("device", 0)] + ([("device_skip", 1)] if ck else []):
            d_out.zero_()
            device(flags)
            assert torch.equal(d_out, d_data), "decoded bytes differ from the input"
            s0 = dev_stats(L)
            row[name + "_GBps"] = timed(lambda: device(flags), data.size)
            row[name + "_stats_delta"] = [y - x for x, y in zip(s0, dev_stats(L))]

        # (c) the block decoder on the same blocks, already in slots
        n, fb = C.c_size_t(0), C.c_size_t(0)
        assert L.LizardGPU_frameIndex(frame.ctypes.data, frame.size, None, None, None, 0, C.byref(n), C.byref(fb)) == 0
        nrec = n.value
        offs, words = np.empty(nrec, dtype=np.uint64), np.empty(nrec, dtype=np.uint32)
        assert L.LizardGPU_frameIndex(frame.ctypes.data, frame.size, None, offs.ctypes.data, words.ctypes.data, nrec, C.byref(n), C.byref(fb)) == 0
        assert not (words >> 31).any(), "a stored-raw record: not a block the block decoder takes"
        stride = (int(words.max()) + 63) & ~63
        slots = np.zeros(nrec * stride, dtype=np.uint8)
        for i in range(nrec):
            slots[i * stride:i * stride + int(words[i])] = frame[int(offs[i]):int(offs[i]) + int(words[i])]
        d_slots = torch.from_numpy(slots).cuda()
        d_sizes = torch.from_numpy(words.astype(np.int32)).cuda()
        d_outsz = torch.zeros(nrec, dtype=torch.int32, device="cuda")

        def blocks():
            rc = L.LizardGPU_decompressBlocks_device(d_slots.data_ptr(), stride, d_sizes.data_ptr(), nrec, d_out.data_ptr(), block, d_outsz.data_ptr(), stream)
            assert rc == 0, L.LizardGPU_lastError()
        d_out.zero_()
        blocks()
        torch.cuda.synchronize()
        assert torch.equal(d_out, d_data), "decoded bytes differ from the input"
        row["blocks_GBps"] = timed(blocks, data.size)
        del d_slots, slots

        # (d) the walk alone
        def walk():
            k, b = C.c_size_t(0), C.c_size_t(0)
            assert L.LizardGPU_frameIndex_device(d_frame.data_ptr(), d_frame.numel(), None, None, None, 0, C.byref(k), C.byref(b), stream) == 0
            assert (k.value, b.value) == (nrec, frame.size)
        w = timed(walk, data.size)
        row["records"] = nrec
        row["walk_ms"] = w["median_ms"]
        row["walk_ns_per_record"] = round(w["median_ms"] * 1e6 / nrec, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_frame
    result = {"input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "repeats": REPS, "warmups": WARM,
              "unit": "GB/s of decoded output, wall clock around a call that ends in a device synchronise",
              "walk_records_per_segment": int(L.LizardGPU_frameWalkRecords()), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
