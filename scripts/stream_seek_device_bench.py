#!/usr/bin/env python3
"""Seekable streams in device memory: what the seek table at the end of a stream buys its reader and costs its writer; same process,
same input, the paths ALTERNATING repetition by repetition.

Input: --mib (default 1024) MiB of the tools generator's output at P50 (16 MiB pieces, consecutive seeds) in device memory, as frames
of 1 MiB and as frames of 64 KiB of input (block size id 1), levels 10 and 30, no checksum.  Wall clock around calls that end in a
device synchronise, GB/s of DECODED (readers) or SOURCE (writers) bytes, median of 5 after 2 warm-ups, with min and max: the spread of
the five is the margin any comparison of two columns has.
  readers, all three on the SAME seekable stream:
    seek     LizardGPU_decompressSeekableStream_device (the table, one batch)
    walk     LizardGPU_decompressStream_device (the serial walk, then one batch; it steps over the table)
    batch    LizardGPU_decompressFrames_device given the frames' pointers, which a holder of a stream does not have: the ceiling
  writers, into one preallocated buffer:
    seekable LizardGPU_compressSeekableStream_device     plain   LizardGPU_compressStream_device
  tensor streams: --tensors (default 1024) bf16 tensors of 1 MiB (weights-like: randn * 0.02), compress_tensors_device(seekable=True),
    then decompress_tensors_device with seek=True and without, and select= of every 64th tensor.
Every reader's output must be the input, byte for byte; LizardGPU_seekDeviceStats must show the table's path in every timed call.
Writes profiles/stream_seek_device.json.

    python scripts/stream_seek_device_bench.py [--mib 1024] [--tensors 1024] [--out profiles/stream_seek_device.json]
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

from lizard_amd import _lib, api
import frame_decode_bench as hb

WARM, REPS = 2, 5


def alternating(paths, nbytes):
    """paths: {name: fn}.  Repetition by repetition every path once, in order; the first WARM repetitions are dropped."""
    t = {k: [] for k in paths}
    for i in range(WARM + REPS):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARM:
                t[k].append(time.perf_counter() - t0)
    out = {}
    for k, v in t.items():
        rate = [nbytes / x / 1e9 for x in v]
        out[k] = {"median": round(statistics.median(rate), 3), "min": round(min(rate), 3), "max": round(max(rate), 3),
                  "median_ms": round(statistics.median(v) * 1e3, 3)}
    return out


def seek_stats(L):
    s = (C.c_ulonglong * 4)()
    assert L.LizardGPU_seekDeviceStats(s) == 0
    return list(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--tensors", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_seek_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    L = _lib.lib()
    data = hb.gen_input(a.mib << 20)
    n = int(data.size)
    d_data = torch.from_numpy(data).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    used, nframes, decoded = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rows = []
    for each in (1 << 20, 64 << 10):
        count = n // each
        views = [d_data[i * each:(i + 1) * each] for i in range(count)]
        for lv in (10, 30):
            row = {"frame_input_bytes": each, "frames": count, "level": lv, "checksum": False}
            d_stream, offs = api.compress_stream_device_into(views, level=lv, block_size_id=1, seekable=True)
            d_stream = d_stream.clone()                         # (the view keeps a bound-sized allocation alive otherwise)
            sbytes, table_at = int(d_stream.numel()), offs[count]
            row["stream_bytes"], row["table_bytes"] = sbytes, sbytes - table_at

            def reader(name, frames_want):
                def fn():
                    r = getattr(L, name)(out.data_ptr(), n, d_stream.data_ptr(), sbytes, C.byref(used), C.byref(nframes), C.byref(decoded), 0, stream)
                    assert r == n and (used.value, nframes.value, decoded.value) == (sbytes, frames_want, n), (name, r, L.LizardGPU_lastError())
                return fn
            srcs = (C.c_void_p * count)(*[d_stream.data_ptr() + o for o in offs[:count]])
            sizes = (C.c_size_t * count)(*[offs[i + 1] - offs[i] for i in range(count)])
            dsts = (C.c_void_p * count)(*[out.data_ptr() + i * each for i in range(count)])
            caps = (C.c_size_t * count)(*([each] * count))
            results, consumed = (C.c_size_t * count)(), (C.c_size_t * count)()

            def batch():
                rc = L.LizardGPU_decompressFrames_device(count, dsts, caps, srcs, sizes, results, consumed, 0, stream)
                assert rc == 0, (rc, L.LizardGPU_lastError())
            paths = {"seek": reader("LizardGPU_decompressSeekableStream_device", count + 1), "walk": reader("LizardGPU_decompressStream_device", count + 1),
                     "batch": batch}
            for k, fn in paths.items():                         # every path decodes to the input
                out.zero_()
                fn()
                assert torch.equal(out, d_data), k
            s0 = seek_stats(L)
            row["readers_GBps"] = alternating(paths, n)
            grown = [y - x for x, y in zip(s0, seek_stats(L))]
            assert grown[:2] == [WARM + REPS, 0], ("the seekable entry fell back", grown)
            r = row["readers_GBps"]
            row["seek_over_walk"] = round(r["seek"]["median"] / r["walk"]["median"], 3)
            row["seek_over_batch"] = round(r["seek"]["median"] / r["batch"]["median"], 3)
            row["seek_not_slower_than_walk_within_spread"] = r["seek"]["max"] >= r["walk"]["min"]

            # the writers, into one buffer that fits either
            cap = sbytes + 4096
            dst = torch.empty(cap, dtype=torch.uint8, device="cuda")

            def writer(seekable):
                def fn():
                    got, _ = api.compress_stream_device_into(views, dst=dst, level=lv, block_size_id=1, seekable=seekable)
                    assert int(got.numel()) == (sbytes if seekable else table_at)
                return fn
            row["writers_GBps"] = alternating({"seekable": writer(True), "plain": writer(False)}, n)
            w = row["writers_GBps"]
            row["seekable_over_plain_writer"] = round(w["seekable"]["median"] / w["plain"]["median"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_stream, dst
        del views
    del out, d_data

    # tensor streams
    g = torch.Generator(device="cuda").manual_seed(7)
    tensors = [(torch.randn(512 * 1024, generator=g, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(a.tensors)]
    tbytes = sum(t.numel() * t.element_size() for t in tensors)
    t_stream = api.compress_tensors_device(tensors, level=10, seekable=True).clone()
    select = list(range(0, a.tensors, 64))
    for kw in (dict(seek=True), dict(), dict(select=select)):
        back = api.decompress_tensors_device(t_stream, **kw)
        want = tensors if "select" not in kw else [tensors[k] for k in select]
        assert len(back) == len(want) and all(torch.equal(b, t) for b, t in zip(back, want)), kw
        del back
    s0 = seek_stats(L)
    tens = alternating({"seek": lambda: api.decompress_tensors_device(t_stream, seek=True), "walk": lambda: api.decompress_tensors_device(t_stream)}, tbytes)
    grown = [y - x for x, y in zip(s0, seek_stats(L))]
    assert grown[:2] == [WARM + REPS, 0], ("decompress_tensors_device(seek=True) fell back", grown)
    sel = alternating({"select": lambda: api.decompress_tensors_device(t_stream, select=select)}, len(select) * (1 << 20))
    tensor_row = {"tensors": a.tensors, "dtype": "bfloat16", "tensor_bytes": 1 << 20, "level": 10, "planes": "bytes", "stream_bytes": int(t_stream.numel()),
                  "decompress_tensors_GBps": tens, "seek_over_walk": round(tens["seek"]["median"] / tens["walk"]["median"], 3),
                  "select_every_64th": {"tensors": len(select), "GBps_of_selected_bytes": sel["select"]}}
    print(json.dumps(tensor_row), flush=True)
    result = {"input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "block_size_id": 1,
              "unit": "GB/s of decoded (readers) or source (writers) bytes, wall clock around calls that end in a device synchronise",
              "method": "median of %d after %d warm-ups, the paths alternating repetition by repetition in one process" % (REPS, WARM),
              "args": {"mib": a.mib, "tensors": a.tensors}, "rows": rows, "tensor_stream": tensor_row}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
