#!/usr/bin/env python3
"""The plane split / join of device buffers (LizardGPU_splitPlanes_device / LizardGPU_joinPlanes_device, planes_kernels.h) against a
device-to-device copy of the same bytes in the same process, and what the split costs and gains end to end.

Part 1.  --mib (default 1024) MiB in device memory as ONE buffer, as buffers of 1 MiB and as buffers of 64 KiB (all 256-byte aligned,
so every 16-byte access of the kernels is aligned), element sizes 2 and 4, split and join, through the C entries with the host arrays
and the destination prepared once.  Each call sits between two events on torch's current stream; GB/s of payload (bytes moved once,
not read plus written), median of 5 after 2 warm-ups, beside the wall clock of the same calls (the entries are synchronous: table
built on the host, uploaded, one wait).  `copy`: dst.copy_(src) of the whole buffer, timed the same way — the yardstick.
Part 2.  The same bytes as bf16 values randn * 0.02 (generated on the device), as tensors of 1 MiB: api.compress_tensors_device /
decompress_tensors_device (split, one tensor header per tensor) against api.compress_stream_device / decompress_stream_device (the
tensors' own bytes), levels 10 and 30, wall clock around calls that end in a device synchronise, GB/s of tensor bytes, median of 5
after 2 warm-ups, and the compressed sizes.  Every round trip must give the input back, bit for bit.
Writes profiles/planes_filter.json.

    python scripts/planes_filter_bench.py [--mib 1024] [--out profiles/planes_filter.json]
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


def timed(fn, nbytes):
    ev, wall = [], []
    for i in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= WARM:
            ev.append(a.elapsed_time(b) * 1e-3)
            wall.append(dt)
    rate = [nbytes / x / 1e9 for x in ev]
    return {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
            "median_ms": round(statistics.median(ev) * 1e3, 3), "wall_median": round(nbytes / statistics.median(wall) / 1e9, 1)}


def wall(fn, nbytes):
    t = []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= WARM:
            t.append(dt)
    rate = [nbytes / x / 1e9 for x in t]
    return out, {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
                 "median_ms": round(statistics.median(t) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_filter.json"))
    args = ap.parse_args()
    L = _lib.lib()
    total = args.mib << 20
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.empty(total // 2, dtype=torch.bfloat16, device=dev)
    step = 1 << 26
    for at in range(0, w.numel(), step):
        n = min(step, w.numel() - at)
        w[at:at + n] = (torch.randn(n, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    src = w.view(torch.uint8)
    dst = torch.empty_like(src)
    back = torch.empty_like(src)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"mib": args.mib, "device": torch.cuda.get_device_name(0), "warm_ups": WARM, "repeats": REPS, "filter": [], "end_to_end": []}
    res["copy"] = timed(lambda: dst.copy_(src), total)
    print("copy", res["copy"], flush=True)
    for what, piece in (("one buffer", total), ("1 MiB buffers", 1 << 20), ("64 KiB buffers", 1 << 16)):
        n = total // piece
        arr = lambda t, base: (t * n)(*[base + i * piece for i in range(n)])
        sizes = (C.c_size_t * n)(*([piece] * n))
        for E in (2, 4):
            elems = (C.c_uint32 * n)(*([E] * n))
            a_src, a_dst, a_back = arr(C.c_void_p, src.data_ptr()), arr(C.c_void_p, dst.data_ptr()), arr(C.c_void_p, back.data_ptr())

            def split():
                _lib.check(L.LizardGPU_splitPlanes_device(n, a_dst, a_src, sizes, elems, stream), "LizardGPU_splitPlanes_device")

            def join():
                _lib.check(L.LizardGPU_joinPlanes_device(n, a_back, a_dst, sizes, elems, stream), "LizardGPU_joinPlanes_device")
            row = {"shape": what, "buffers": n, "elem_size": E, "split": timed(split, total), "join": timed(join, total)}
            assert torch.equal(back, src), "join(split(x)) != x"
            row["split_of_copy"] = round(row["split"]["median"] / res["copy"]["median"], 3)
            row["join_of_copy"] = round(row["join"]["median"] / res["copy"]["median"], 3)
            res["filter"].append(row)
            print(row, flush=True)
    del dst, back
    tensors = [w[i:i + (1 << 19)] for i in range(0, w.numel(), 1 << 19)]
    raw = [t.view(torch.uint8) for t in tensors]
    for level in (10, 30):
        s_split, c_split = wall(lambda: api.compress_tensors_device(tensors, level=level), total)
        s_plain, c_plain = wall(lambda: api.compress_stream_device(raw, level=level), total)
        out, d_split = wall(lambda: api.decompress_tensors_device(s_split), total)
        (plain, _), d_plain = wall(lambda: api.decompress_stream_device(s_plain, size=total), total)
        assert len(out) == len(tensors) and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(out, tensors))
        assert torch.equal(plain, src)
        row = {"level": level, "tensors": len(tensors), "tensor_bytes": 1 << 20,
               "split": {"compress": c_split, "decompress": d_split, "stream_bytes": int(s_split.numel()), "ratio": round(s_split.numel() / total, 4)},
               "unsplit": {"compress": c_plain, "decompress": d_plain, "stream_bytes": int(s_plain.numel()), "ratio": round(s_plain.numel() / total, 4)}}
        res["end_to_end"].append(row)
        print(row, flush=True)
        del s_split, s_plain, out, plain
    st = (C.c_ulonglong * 4)()
    assert L.LizardGPU_planesStats(st) == 0
    res["planes_stats"] = list(st)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
