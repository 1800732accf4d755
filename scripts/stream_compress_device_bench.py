#!/usr/bin/env python3
"""A .liz stream of many device buffers written into ONE device buffer: api.compress_stream_device_into (one call of
LizardGPU_compressStream_device, every byte written once, to its place) against api._compress_stream_device_cat (the way before that
entry: LizardGPU_compressFrames_device into bound-sized regions, then one torch.cat) and against the block kernels on the same bytes;
same process, same input, the two stream paths alternating inside the timed loop.

Input: --mib (default 1024) MiB of the tools generator's output at P50 (16 MiB pieces, consecutive seeds) in device memory, seen as
buffers of 1 MiB and as buffers of 64 KiB (views of the one tensor).  Levels 10 and 30, block size id 1, with and without content
checksum.  Wall clock around calls that end in a device synchronise, GB/s of INPUT, median of 5 after 2 warm-ups, min-max beside it.
  (a) into     api.compress_stream_device_into, no dst: one allocation of LizardGPU_compressStreamBound bytes, one call
  (b) cat      api._compress_stream_device_cat
  (c) blocks   LizardGPU_compressBlocks_device on the same bytes (blocks of 128 KiB, or of 64 KiB for the 64 KiB buffers): bound-sized
               slots and a size array, no frames: the ceiling
The streams of (a) and (b) must be the same bytes, and (a)'s must decode to the input with decompress_stream_device.  For (a) and (b)
torch.cuda.max_memory_allocated over one call, less what was allocated before it, is recorded as peak_extra_bytes.
Tensor streams: api.compress_tensors_device on --mib bf16 tensors of 1 MiB (randn * 0.02), levels 10 and 30, against the old
composition (split, _compress_frames_device, the headers uploaded, one torch.cat), same bytes required.
Writes profiles/stream_compress_device.json, with the command line in the file.

    python scripts/stream_compress_device_bench.py [--mib 1024] [--out profiles/stream_compress_device.json]
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

from lizard_amd import _lib, api
import frame_decode_bench as hb

BLOCK = 128 << 10
WARM, REPS = 2, 5


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(t, nbytes):
    rate = [nbytes / x / 1e9 for x in t]
    return {"median": round(statistics.median(rate), 3), "min": round(min(rate), 3), "max": round(max(rate), 3),
            "median_ms": round(statistics.median(t) * 1e3, 3)}


def alternating(fns, nbytes):
    """Every function WARM + REPS times, taking turns; the summaries in the functions' order."""
    times = [[] for _ in fns]
    for i in range(WARM + REPS):
        for k, fn in enumerate(fns):
            dt = once(fn)
            if i >= WARM:
                times[k].append(dt)
    return [summary(t, nbytes) for t in times]


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def old_tensor_stream(tensors, level):
    """compress_tensors_device as it was before the stream entry (byte planes, no checksum)."""
    L = _lib.lib()
    raw = [api._as_bytes(t) for t in tensors]
    elems = [api._plane_elem_size(t) for t in tensors]
    raw = api.split_planes_device(raw, elems)
    frames = api._compress_frames_device(raw, level, 0, False, True, api.STREAM_FRAME_SLACK)
    host = np.zeros(len(tensors) * api.TENSOR_HEADER_MAX, dtype=np.uint8)
    at, spans = 0, []
    for t, e in zip(tensors, elems):
        d = api._TensorDesc()
        d.elemSize, d.ndim, d.nbytes, d.dtype = e, t.dim(), int(t.numel()) * t.element_size(), str(t.dtype).split(".")[-1].encode()
        d.filter = api.FILTER_BYTE_PLANES
        for k, s in enumerate(t.shape):
            d.shape[k] = int(s)
        n = L.LizardGPU_tensorHeaderWrite2(host.ctypes.data + at, host.size - at, C.byref(d))
        assert n
        spans.append((at, at + n))
        at += n
    headers = torch.from_numpy(host[:at]).to(tensors[0].device)
    return torch.cat([x for (a, b), f in zip(spans, frames) for x in (headers[a:b], f)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_compress_device.json"))
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
        views = [d_data[i * each:(i + 1) * each] for i in range(count)]
        for lv, ck in [(lv, ck) for lv in (10, 30) for ck in (False, True)]:
            row = {"buffer_bytes": each, "buffers": count, "level": lv, "checksum": ck}
            into = lambda: api.compress_stream_device_into(views, level=lv, block_size_id=1, checksum=ck)[0]
            cat = lambda: api._compress_stream_device_cat(views, level=lv, block_size_id=1, checksum=ck)
            new, old = into(), cat()
            assert torch.equal(new, old), "the two paths wrote different streams"
            back, frames = api.decompress_stream_device(new)
            assert frames == count and torch.equal(back, d_data[:count * each]), "the stream does not decode to the input"
            row["stream_bytes"] = int(new.numel())
            del new, old, back
            row["into_GBps"], row["cat_GBps"] = alternating([into, cat], count * each)
            row["into_peak_extra_bytes"], row["cat_peak_extra_bytes"] = peak_extra(into), peak_extra(cat)

            block = min(BLOCK, each)
            nb = n // block
            stride = (api.Lizard_compressBound(block) + 63) & ~63
            d_slots = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(nb, dtype=torch.int32, device="cuda")

            def blocks():
                rc = L.LizardGPU_compressBlocks_device(d_data.data_ptr(), nb, block, block, d_slots.data_ptr(), stride, d_sizes.data_ptr(), lv, stream)
                assert rc == 0, L.LizardGPU_lastError()
            row["blocks_GBps"] = alternating([blocks], n)[0]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_slots, d_sizes
        del views
    del d_data

    # tensor streams: bf16 tensors of 1 MiB
    g = torch.Generator().manual_seed(1)
    tensors = [(torch.randn(512, 1024, generator=g) * 0.02).to(torch.bfloat16).cuda() for _ in range(a.mib)]
    trows = []
    for lv in (10, 30):
        new_fn = lambda: api.compress_tensors_device(tensors, level=lv)
        old_fn = lambda: old_tensor_stream(tensors, lv)
        new, old = new_fn(), old_fn()
        assert torch.equal(new, old), "compress_tensors_device and the old composition wrote different streams"
        r = {"tensors": len(tensors), "tensor_bytes": 1 << 20, "dtype": "bfloat16", "level": lv, "stream_bytes": int(new.numel())}
        del new, old
        r["new_GBps"], r["old_GBps"] = alternating([new_fn, old_fn], len(tensors) << 20)
        r["new_peak_extra_bytes"], r["old_peak_extra_bytes"] = peak_extra(new_fn), peak_extra(old_fn)
        trows.append(r)
        print(json.dumps(r), flush=True)
    result = {"command": " ".join(sys.argv), "input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "block_size_id": 1,
              "unit": "GB/s of input, wall clock around calls that end in a device synchronise; new and old alternate inside the loop",
              "repeats": [WARM, REPS], "rows": rows, "tensor_streams": trows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
