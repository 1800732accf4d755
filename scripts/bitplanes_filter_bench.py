#!/usr/bin/env python3
"""The bit-plane split / join of device buffers (LizardGPU_splitBitPlanes_device / LizardGPU_joinBitPlanes_device, bitplanes_kernels.h)
against the byte-plane split / join (planes_kernels.h) and a device-to-device copy of the same bytes, all in the same process, and
what either filter costs and gains end to end.

Part 1.  --mib (default 1024) MiB in device memory as ONE buffer, as buffers of 1 MiB and as buffers of 64 KiB (all 256-byte aligned),
element sizes 2 and 4, split and join, bits and bytes, through the C entries with the host arrays and the destination prepared once.
Each call sits between two events on torch's current stream; GB/s of payload (bytes moved once, not read plus written), median of 5
after 2 warm-ups, beside the wall clock of the same calls (the entries are synchronous).  `copy`: dst.copy_(src) of the whole buffer,
timed the same way, in front of the filters and once more behind them — the yardstick, with the byte filter.
Part 2.  The same number of bytes as bf16 and as fp16 values randn * 0.02 (generated on the device), as tensors of 1 MiB:
api.compress_tensors_device / decompress_tensors_device with planes="bytes" against planes="bits", levels 10 and 30, wall clock
around calls that end in a device synchronise, GB/s of tensor bytes, median of 5 after 2 warm-ups, and stream / raw.  Every round trip
must give the input back, bit for bit.
Writes profiles/bitplanes_filter.json.

    python scripts/bitplanes_filter_bench.py [--mib 1024] [--out profiles/bitplanes_filter.json]
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


def weights(total, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.empty(total // 2, dtype=dtype, device=dev)
    step = 1 << 26
    for at in range(0, w.numel(), step):
        n = min(step, w.numel() - at)
        w[at:at + n] = (torch.randn(n, generator=g, device=dev) * 0.02).to(dtype)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitplanes_filter.json"))
    args = ap.parse_args()
    L = _lib.lib()
    total = args.mib << 20
    dev = torch.device("cuda")
    w = weights(total, torch.bfloat16, dev)
    src = w.view(torch.uint8)
    dst = torch.empty_like(src)
    back = torch.empty_like(src)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"mib": args.mib, "device": torch.cuda.get_device_name(0), "warm_ups": WARM, "repeats": REPS, "filter": [], "end_to_end": []}
    res["copy"] = timed(lambda: dst.copy_(src), total)
    print("copy", res["copy"], flush=True)
    entries = {"bits": (L.LizardGPU_splitBitPlanes_device, L.LizardGPU_joinBitPlanes_device),
               "bytes": (L.LizardGPU_splitPlanes_device, L.LizardGPU_joinPlanes_device)}
    for what, piece in (("one buffer", total), ("1 MiB buffers", 1 << 20), ("64 KiB buffers", 1 << 16)):
        n = total // piece
        arr = lambda t, base: (t * n)(*[base + i * piece for i in range(n)])
        sizes = (C.c_size_t * n)(*([piece] * n))
        for E in (2, 4):
            elems = (C.c_uint32 * n)(*([E] * n))
            a_src, a_dst, a_back = arr(C.c_void_p, src.data_ptr()), arr(C.c_void_p, dst.data_ptr()), arr(C.c_void_p, back.data_ptr())
            row = {"shape": what, "buffers": n, "elem_size": E}
            for planes, (f_split, f_join) in entries.items():
                def split():
                    _lib.check(f_split(n, a_dst, a_src, sizes, elems, stream), "split " + planes)

                def join():
                    _lib.check(f_join(n, a_back, a_dst, sizes, elems, stream), "join " + planes)
                back.zero_()
                r = {"split": timed(split, total), "join": timed(join, total)}
                assert torch.equal(back, src), "join(split(x)) != x"
                r["split_of_copy"] = round(r["split"]["median"] / res["copy"]["median"], 3)
                r["join_of_copy"] = round(r["join"]["median"] / res["copy"]["median"], 3)
                row[planes] = r
            row["bits_of_bytes"] = {k: round(row["bits"][k]["median"] / row["bytes"][k]["median"], 3) for k in ("split", "join")}
            res["filter"].append(row)
            print(row, flush=True)
    res["copy_after"] = timed(lambda: dst.copy_(src), total)     # the yardstick once more, behind the filters
    print("copy again", res["copy_after"], flush=True)
    del dst, back, src
    for name, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        if dtype != torch.bfloat16:
            del w
            w = weights(total, dtype, dev)
        tensors = [w[i:i + (1 << 19)] for i in range(0, w.numel(), 1 << 19)]
        for level in (10, 30):
            row = {"data": name + " randn * 0.02", "level": level, "tensors": len(tensors), "tensor_bytes": 1 << 20}
            for planes in ("bytes", "bits"):
                s, c = wall(lambda: api.compress_tensors_device(tensors, level=level, planes=planes), total)
                out, d = wall(lambda: api.decompress_tensors_device(s), total)
                assert len(out) == len(tensors) and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(out, tensors))
                row[planes] = {"compress": c, "decompress": d, "stream_bytes": int(s.numel()), "ratio": round(s.numel() / total, 4)}
                del s, out
            res["end_to_end"].append(row)
            print(row, flush=True)
    st = (C.c_ulonglong * 4)()
    assert L.LizardGPU_bitPlanesStats(st) == 0
    res["bit_planes_stats"] = list(st)
    assert L.LizardGPU_planesStats(st) == 0
    res["planes_stats"] = list(st)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
