#!/usr/bin/env python3
"""A STREAM of frames in device memory — back to back in one buffer, no table of pointers — decoded into device memory:
LizardGPU_decompressStream_device against the two things a caller can do with the same bytes; same process, same input.

Input: --mib (default 1024) MiB of the tools generator's output at P50 (16 MiB pieces, consecutive seeds) in device memory, compressed
by api.compress_stream_device (LizardGPU_compressFrames_device with content size, frames joined by torch.cat) into frames of 1 MiB and
into frames of 64 KiB of input (block size id 1, so 8 records or 1 record per frame).  Levels 10 and 30, with and without content
checksum (verified where there is one).  Wall clock around calls that end in a device synchronise, GB/s of DECODED bytes, median of 5
(and min-max), 2 warm-ups.
  stream   LizardGPU_decompressStream_device, one call on the whole stream
  (a) loop     LizardGPU_decompressFrame_device called again and again with the consumed bytes, the only way to decode the stream
               without the entry: 1 warm-up, 3 timed repeats, over the first --loop-frames (default 2048) frames only; its rate is per
               decoded byte of the frames it covered
  (b) batch    LizardGPU_decompressFrames_device given the frames' pointers and sizes (which a holder of a stream does not have): the
               ceiling
  walk     LizardGPU_streamIndex_device alone: the serial walk across frame boundaries, microseconds per frame
  single   one frame of the whole input without content size (block size id 1), what the reference's CLI writes by default: stream
           entry against one LizardGPU_decompressFrame_device call, level 10, no checksum
The output of every method must be the input, byte for byte.  The growth of LizardGPU_streamDecodeDeviceStats over the timed repeats of
the stream entry is recorded ([1] must be one batch per call, [2] must stay 0).
Writes profiles/stream_decode_device.json.

    python scripts/stream_decode_device_bench.py [--mib 1024] [--loop-frames 2048] [--out profiles/stream_decode_device.json]
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


def stream_stats(L):
    s = (C.c_ulonglong * 4)()
    assert L.LizardGPU_streamDecodeDeviceStats(s) == 0
    return list(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--loop-frames", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_decode_device.json"))
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
        covered = min(count, a.loop_frames)
        for lv, ck in [(lv, ck) for lv in (10, 30) for ck in (0, 1)]:
            row = {"frame_input_bytes": each, "frames": count, "level": lv, "checksum": bool(ck)}
            frames = api.compress_frames_device([d_data[i * each:(i + 1) * each] for i in range(count)], level=lv, block_size_id=1, checksum=bool(ck),
                                                content_size=True)
            d_stream = torch.cat(frames)
            sbytes = int(d_stream.numel())
            sizes_py = [int(f.numel()) for f in frames]
            del frames
            row["stream_bytes"] = sbytes

            # the stream entry
            def whole():
                r = L.LizardGPU_decompressStream_device(out.data_ptr(), n, d_stream.data_ptr(), sbytes, C.byref(used), C.byref(nframes), C.byref(decoded), 0, stream)
                assert r == n, (r, L.LizardGPU_lastError())
            out.zero_()
            whole()
            assert (used.value, nframes.value, decoded.value) == (sbytes, count, n), L.LizardGPU_lastError()
            assert torch.equal(out, d_data), "the stream entry does not decode to the input"
            s0 = stream_stats(L)
            row["stream_GBps"] = timed(whole, n, 2, 5)
            row["stream_stats_delta"] = [y - x for x, y in zip(s0, stream_stats(L))]
            assert row["stream_stats_delta"][1] == 7 and row["stream_stats_delta"][2] == 0, "not one batch per call, or a frame was handed over"

            # the walk alone
            nf, total = C.c_size_t(0), C.c_size_t(0)

            def walk():
                rc = L.LizardGPU_streamIndex_device(d_stream.data_ptr(), sbytes, None, None, None, None, 0, C.byref(nf), C.byref(total), stream)
                assert rc == 0, (rc, L.LizardGPU_lastError())
            w = timed(walk, n, 2, 5)
            assert (nf.value, total.value) == (count, sbytes)
            row["walk_ms"] = w["median_ms"]
            row["walk_us_per_frame"] = round(w["median_ms"] * 1e3 / count, 3)
            row["walk_share_of_stream"] = round(w["median_ms"] / row["stream_GBps"]["median_ms"], 3)

            # (a) the loop over the single-frame entry, on the stream
            out.zero_()

            def loop():
                pos, at = 0, 0
                for _ in range(covered):
                    r = L.LizardGPU_decompressFrame_device(out.data_ptr() + at, n - at, d_stream.data_ptr() + pos, sbytes - pos, C.byref(used), 0, stream)
                    assert r == each, (r, L.LizardGPU_lastError())
                    at += r
                    pos += used.value
            row["loop_frames"] = covered
            row["loop_GBps"] = timed(loop, covered * each, 1, 3)
            assert torch.equal(out[:covered * each], d_data[:covered * each]), "the loop does not decode to the input"

            # (b) the batch entry, given the pointers
            offs, pos = [], 0
            for s in sizes_py:
                offs.append(pos)
                pos += s
            srcs = (C.c_void_p * count)(*[d_stream.data_ptr() + o for o in offs])
            sizes = (C.c_size_t * count)(*sizes_py)
            dsts = (C.c_void_p * count)(*[out.data_ptr() + i * each for i in range(count)])
            caps = (C.c_size_t * count)(*([each] * count))
            results, consumed = (C.c_size_t * count)(), (C.c_size_t * count)()

            def batch():
                rc = L.LizardGPU_decompressFrames_device(count, dsts, caps, srcs, sizes, results, consumed, 0, stream)
                assert rc == 0, (rc, L.LizardGPU_lastError())
            out.zero_()
            batch()
            assert all(r == each for r in results) and torch.equal(out, d_data), "the batch does not decode to the input"
            row["batch_GBps"] = timed(batch, n, 2, 5)
            row["stream_over_loop"] = round(row["stream_GBps"]["median"] / row["loop_GBps"]["median"], 2)
            row["stream_over_batch"] = round(row["stream_GBps"]["median"] / row["batch_GBps"]["median"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del d_stream

    # one frame without content size: what a file made by the reference's CLI is
    one = api.compress_frames_device([d_data], level=10, block_size_id=1, checksum=False, content_size=False)[0]
    obytes = int(one.numel())

    def one_stream():
        r = L.LizardGPU_decompressStream_device(out.data_ptr(), n, one.data_ptr(), obytes, C.byref(used), C.byref(nframes), None, 0, stream)
        assert r == n, (r, L.LizardGPU_lastError())

    def one_single():
        r = L.LizardGPU_decompressFrame_device(out.data_ptr(), n, one.data_ptr(), obytes, C.byref(used), 0, stream)
        assert r == n, (r, L.LizardGPU_lastError())
    out.zero_()
    one_stream()
    assert (used.value, nframes.value) == (obytes, 1) and torch.equal(out, d_data)
    single = {"frame_bytes": obytes, "level": 10, "checksum": False, "content_size": False,
              "stream_GBps": timed(one_stream, n, 2, 5), "single_entry_GBps": timed(one_single, n, 2, 5)}
    print(json.dumps(single), flush=True)
    result = {"input_MiB": a.mib, "input": "tools datagen P50, 16 MiB pieces, seeds 1000..", "block_size_id": 1,
              "unit": "GB/s of decoded bytes, wall clock around calls that end in a device synchronise",
              "repeats": {"stream": [2, 5], "walk": [2, 5], "loop": [1, 3], "batch": [2, 5]},
              "args": {"mib": a.mib, "loop_frames": a.loop_frames}, "LIZARDGPU_STREAM_WALK_FRAMES": os.environ.get("LIZARDGPU_STREAM_WALK_FRAMES"),
              "rows": rows, "single_frame_stream": single}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
