#!/usr/bin/env python3
"""A row range of every tensor of a seekable tensor stream in device memory: what decoding only the covering blocks buys a sharded
loader in time and in memory; same process, same stream, the two paths ALTERNATING repetition by repetition.

Input: --tensors (default 64) bf16 tensors of (--rows 8192, --cols 1024) — 1 GiB in all, weights-like: randn * 0.02 —,
compress_tensors_device(seekable=True), byte planes, levels 10 and 30, the default block size (128 KiB).  For rows
[rank * rows / 8, (rank + 1) * rows / 8) of EVERY tensor (--rank, default 3; --parts, default 8):
    slice    api.decompress_tensor_slices_device            (the covering blocks alone, then the range join)
    whole    api.decompress_tensors_device(seek=True), then [start:stop] of every tensor
Wall clock around calls that end in a device synchronise, median of 5 after 2 warm-ups with min and max, and
torch.cuda.max_memory_allocated beyond what is allocated before the call (the stream and the tensors stay allocated throughout).
Both outputs must equal the source rows, bit for bit.  LizardGPU_sliceDeviceStats gives the records the slice path decoded.
The one expectation that can be derived is memory: scratch + result of the slice path is about 2 / parts of the tensors' bytes plus at
most two blocks per plane per tensor, against about twice the tensors' bytes for the whole path.  The walk of a frame's record chain
stays serial, one wave per frame (0.27 us per record measured for the single-frame walk): at 128 KiB blocks the walk, not the decode,
may bound the slice of one very large tensor; the rows of the JSON say what was measured.
Writes profiles/tensor_slice_device.json.

    python scripts/tensor_slice_device_bench.py [--tensors 64] [--rows 8192] [--cols 1024] [--out profiles/tensor_slice_device.json]
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
import torch

from lizard_amd import _lib, api

WARM, REPS = 2, 5


def measure(paths):
    """paths: {name: fn}.  Repetition by repetition every path once, in order; the first WARM repetitions are dropped.  Per path the
    wall-clock seconds and the peak of allocated device memory beyond what was allocated before the call."""
    t, peak = {k: [] for k in paths}, {k: 0 for k in paths}
    for i in range(WARM + REPS):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - before)
            del out
            if i >= WARM:
                t[k].append(dt)
    return {k: {"median_ms": round(statistics.median(v) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3),
                "peak_bytes_beyond_the_stream": int(peak[k])} for k, v in t.items()}


STEPS = ("LizardGPU_seekTable_device", "LizardGPU_framesInfo_device", "LizardGPU_decompressFrameRanges_device", "LizardGPU_joinPlanesRange_device")


def breakdown(L, fn):
    """Where the slice path's time goes, outside the timed repetitions: wall clock of each C entry it calls (every one of them ends in
    a host wait), median of REPS repetitions; "python" is the rest of the call (the header read, ctypes, the allocations)."""
    spent = {k: [] for k in STEPS}
    total = []
    saved = {k: getattr(L, k) for k in STEPS}

    def timed(name):
        def call(*args):
            t0 = time.perf_counter()
            r = saved[name](*args)
            spent[name][-1] += time.perf_counter() - t0     # (the sum of the repetition: an entry may be called more than once)
            return r
        return call
    for k in STEPS:
        setattr(L, k, timed(k))
    try:
        for _ in range(REPS):
            for k in STEPS:
                spent[k].append(0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            total.append(time.perf_counter() - t0)
            del out
    finally:
        for k in STEPS:
            setattr(L, k, saved[k])
    out = {k.replace("LizardGPU_", ""): round(statistics.median(v) * 1e3, 3) for k, v in spent.items()}
    out["python"] = round((statistics.median(total) - sum(statistics.median(v) for v in spent.values())) * 1e3, 3)
    return out


def slice_stats(L):
    s = (C.c_ulonglong * 4)()
    assert L.LizardGPU_sliceDeviceStats(s) == 0
    return list(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tensors", type=int, default=64)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_slice_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    tensors = [(torch.randn(a.rows, a.cols, generator=g, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(a.tensors)]
    tbytes = sum(t.numel() * t.element_size() for t in tensors)
    start, stop = a.rank * a.rows // a.parts, (a.rank + 1) * a.rows // a.parts
    sbytes = a.tensors * (stop - start) * a.cols * 2
    slices = [(k, start, stop) for k in range(a.tensors)]
    rows = []
    for lv in (10, 30):
        stream = api.compress_tensors_device(tensors, level=lv, seekable=True).clone()

        def by_slice():
            return api.decompress_tensor_slices_device(stream, slices)

        def by_whole():
            return [t[start:stop] for t in api.decompress_tensors_device(stream, seek=True)]
        for name, fn in (("slice", by_slice), ("whole", by_whole)):
            got = fn()
            assert len(got) == a.tensors and all(torch.equal(x, t[start:stop]) for x, t in zip(got, tensors)), name
            del got
        s0 = slice_stats(L)
        m = measure({"slice": by_slice, "whole": by_whole})
        grown = [y - x for x, y in zip(s0, slice_stats(L))]
        steps = breakdown(L, by_slice)
        row = {"slice_steps_median_ms": steps, "level": lv, "planes": "bytes", "stream_bytes": int(stream.numel()), "paths": m,
               "slice_records_decoded_per_call": grown[0] // (WARM + REPS), "records_in_the_stream": a.tensors * -(-(a.rows * a.cols * 2) // 131072),
               "slice_over_whole_time": round(m["slice"]["median_ms"] / m["whole"]["median_ms"], 3),
               "slice_over_whole_peak_memory": round(m["slice"]["peak_bytes_beyond_the_stream"] / max(m["whole"]["peak_bytes_beyond_the_stream"], 1), 3),
               "slice_GBps_of_sliced_bytes": round(sbytes / m["slice"]["median_ms"] / 1e6, 3),
               "whole_GBps_of_tensor_bytes": round(tbytes / m["whole"]["median_ms"] / 1e6, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del stream
    result = {"tensors": a.tensors, "shape": [a.rows, a.cols], "dtype": "bfloat16", "tensor_bytes_total": tbytes, "rows_sliced": [start, stop],
              "sliced_bytes_total": sbytes, "block_bytes": 131072,
              "unit": "wall clock around calls that end in a device synchronise; torch.cuda.max_memory_allocated beyond what was allocated before the call",
              "method": "median of %d after %d warm-ups, the paths alternating repetition by repetition in one process" % (REPS, WARM),
              "note": "the walk of a frame's record chain is serial, one wave per frame, in both paths; the slice path walks every picked frame twice (count, fill)",
              "args": vars(a), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
