#!/usr/bin/env python3
"""The XOR-with-base split / join of device buffers (LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device) against what a
caller could do without it, all in the same process, and what the filter gains and costs end to end.

Part 1.  --mib (default 1024) MiB in device memory as buffers of 1 MiB (256-byte aligned), beside a base of the same size, element
sizes 2 (bf16) and 4 (fp32), byte planes and bit planes, split and join, through the C entries with the host arrays and the
destinations prepared once.  Four candidates ALTERNATE, one call each per round, 2 warm-up rounds and 5 measured ones; each call sits
between two events on torch's current stream; GB/s of payload (bytes moved once), the median:
  fused      the XOR entry: 3 bytes of memory traffic per payload byte
  xor+plain  torch.bitwise_xor into a temporary and the plain filter (split), or the plain filter into a temporary and
             torch.bitwise_xor (join): what a caller can do without the entry, 5 bytes per payload byte and a third buffer
  plain      the plain filter alone, 2 bytes per payload byte
  copy       dst.copy_(src)
By byte counts `fused` is expected near 2/3 of `plain` and must not be below `xor+plain`.
Part 2.  The same number of bytes as bf16 tensors of 1 MiB, w = randn * 0.02 and w + step with step = 1e-5 * sign(randn) * rand
(generated on the device), the base w: api.compress_tensors_device / decompress_tensors_device with and without `base`, levels 10
and 30, wall clock around calls that end in a device synchronise, GB/s of tensor bytes, median of 5 after 2 warm-ups, stream / raw
and the peak of torch.cuda.max_memory_allocated over the calls.  Every round trip must give the input back, bit for bit.
Writes profiles/planes_xor_filter.json.

    python scripts/planes_xor_bench.py [--mib 1024] [--out profiles/planes_xor_filter.json]
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
PIECE = 1 << 20


def alternate(candidates, nbytes):
    """{name: fn} -> {name: rates}: one call of each per round, in turn."""
    ev = {k: [] for k in candidates}
    for i in range(WARM + REPS):
        for name, fn in candidates.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= WARM:
                ev[name].append(a.elapsed_time(b) * 1e-3)
    out = {}
    for name, t in ev.items():
        rate = [nbytes / x / 1e9 for x in t]
        out[name] = {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
                     "median_ms": round(statistics.median(t) * 1e3, 3)}
    return out


def wall(fn, nbytes):
    t = []
    torch.cuda.reset_peak_memory_stats()
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= WARM:
            t.append(dt)
        if i + 1 < WARM + REPS:
            del out
    rate = [nbytes / x / 1e9 for x in t]
    return out, {"median": round(statistics.median(rate), 1), "min": round(min(rate), 1), "max": round(max(rate), 1),
                 "median_ms": round(statistics.median(t) * 1e3, 3), "peak_allocated_bytes": int(torch.cuda.max_memory_allocated())}


def stepped(total, dev, lr=1e-5):
    """(w + step, w) as bf16, total bytes each, generated on the device from manual_seed(1)."""
    g = torch.Generator(device=dev).manual_seed(1)
    new = torch.empty(total // 2, dtype=torch.bfloat16, device=dev)
    old = torch.empty_like(new)
    chunk = 1 << 26
    for at in range(0, new.numel(), chunk):
        n = min(chunk, new.numel() - at)
        w = torch.randn(n, generator=g, device=dev) * 0.02
        step = lr * torch.sign(torch.randn(n, generator=g, device=dev)) * torch.rand(n, generator=g, device=dev)
        new[at:at + n] = (w + step).to(torch.bfloat16)
        old[at:at + n] = w.to(torch.bfloat16)
    return new, old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_xor_filter.json"))
    args = ap.parse_args()
    L = _lib.lib()
    total = args.mib << 20
    dev = torch.device("cuda")
    new, old = stepped(total, dev)
    src, base = new.view(torch.uint8), old.view(torch.uint8)
    planar, tmp, back = torch.empty_like(src), torch.empty_like(src), torch.empty_like(src)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = total // PIECE
    arr = lambda t: (C.c_void_p * n)(*[t.data_ptr() + i * PIECE for i in range(n)])
    a_src, a_base, a_planar, a_tmp, a_back = arr(src), arr(base), arr(planar), arr(tmp), arr(back)
    sizes = (C.c_size_t * n)(*([PIECE] * n))
    res = {"mib": args.mib, "device": torch.cuda.get_device_name(0), "warm_ups": WARM, "repeats": REPS, "buffers": n, "buffer_bytes": PIECE,
           "filter": [], "end_to_end": []}
    plain = {0: (L.LizardGPU_splitPlanes_device, L.LizardGPU_joinPlanes_device), 1: (L.LizardGPU_splitBitPlanes_device, L.LizardGPU_joinBitPlanes_device)}
    for E in (2, 4):
        elems = (C.c_uint32 * n)(*([E] * n))
        for filt, name in ((0, "bytes"), (1, "bits")):
            p_split, p_join = plain[filt]

            def fused_split():
                _lib.check(L.LizardGPU_splitPlanesXor_device(n, a_planar, a_src, a_base, sizes, elems, filt, stream), "fused split")

            def xor_then_split():
                torch.bitwise_xor(src, base, out=tmp)
                _lib.check(p_split(n, a_planar, a_tmp, sizes, elems, stream), "split")

            def plain_split():
                _lib.check(p_split(n, a_planar, a_src, sizes, elems, stream), "split")

            def fused_join():
                _lib.check(L.LizardGPU_joinPlanesXor_device(n, a_back, a_planar, a_base, sizes, elems, filt, stream), "fused join")

            def join_then_xor():
                _lib.check(p_join(n, a_tmp, a_planar, sizes, elems, stream), "join")
                torch.bitwise_xor(tmp, base, out=back)

            def plain_join():
                _lib.check(p_join(n, a_back, a_planar, sizes, elems, stream), "join")

            row = {"elem_size": E, "planes": name}
            row["split"] = alternate({"fused": fused_split, "xor+plain": xor_then_split, "plain": plain_split, "copy": lambda: back.copy_(src)}, total)
            xor_then_split()
            want = planar.clone()
            fused_split()
            assert torch.equal(planar, want), "the fused split is not split(src ^ base)"
            del want
            row["join"] = alternate({"fused": fused_join, "xor+plain": join_then_xor, "plain": plain_join, "copy": lambda: tmp.copy_(src)}, total)
            back.zero_()
            fused_join()
            assert torch.equal(back, src), "join(split(x, b), b) != x"
            for k in ("split", "join"):
                row[k + "_fused_of_plain"] = round(row[k]["fused"]["median"] / row[k]["plain"]["median"], 3)
                row[k + "_fused_of_xor+plain"] = round(row[k]["fused"]["median"] / row[k]["xor+plain"]["median"], 3)
            res["filter"].append(row)
            print(row, flush=True)
    del planar, tmp, back, src, base
    torch.cuda.empty_cache()
    per = PIECE // 2
    tensors = [new[i:i + per] for i in range(0, new.numel(), per)]
    bases = [old[i:i + per] for i in range(0, old.numel(), per)]
    for level in (10, 30):
        row = {"data": "bf16 randn * 0.02 + step, lr 1e-5", "level": level, "tensors": len(tensors), "tensor_bytes": PIECE}
        for what, kw_c, kw_d in (("without_base", {}, {}), ("with_base", {"base": bases, "base_tag": 1}, {"base": bases, "base_tag": 1})):
            s, c = wall(lambda: api.compress_tensors_device(tensors, level=level, **kw_c), total)
            out, d = wall(lambda: api.decompress_tensors_device(s, **kw_d), total)
            assert len(out) == len(tensors) and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(out, tensors))
            row[what] = {"compress": c, "decompress": d, "stream_bytes": int(s.numel()), "ratio": round(s.numel() / total, 4)}
            del s, out
        res["end_to_end"].append(row)
        print(row, flush=True)
    st = (C.c_ulonglong * 4)()
    assert L.LizardGPU_planesXorStats(st) == 0
    res["planes_xor_stats"] = list(st)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
