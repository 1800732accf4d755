#!/usr/bin/env python3
"""What the bit-plane filter (include/lizard_amd.h Part 3c) gains and loses against the byte-plane filter, on the CPU, without a GPU:
the numpy models of both layouts (tests/bitplanes_inputs.py, tests/planes_inputs.py) and the unmodified reference library under
oracle/_ref (built with -DLIZARD_RESET_MEM, tests/util.py).  Every input is split whole, cut into 128 KiB blocks, each block through
Lizard_compress; a block counts with its compressed size when that is below its own size and with its own size otherwise (what a
frame stores); the sum over raw bytes is the ratio.  Inputs: torch.manual_seed(1); randn(2^19) * 0.02 as fp16, bf16 and fp32 (the
README's table), and the rows where bit planes lose or tie: bf16 randn(2^19) * 1.0, int32 indices below 50 000, int64 arange(2^17),
and a bf16 tensor of 8 KiB.  Levels 10, 21, 30, 41.  Writes profiles/bitplanes_ratio.json.

    python scripts/bitplanes_ratio.py [--out profiles/bitplanes_ratio.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bitplanes_inputs as bi
import planes_inputs as pi
import util

BLOCK = 128 << 10
LEVELS = (10, 21, 30, 41)


def stored_bytes(ref, data, level):
    """The bytes a frame of 128 KiB blocks holds for `data` (a uint8 array), without the frame's own header and block headers."""
    total = 0
    cap = ref.Lizard_compressBound(BLOCK)
    dst = C.create_string_buffer(cap)
    for at in range(0, data.size, BLOCK):
        block = np.ascontiguousarray(data[at:at + BLOCK])
        c = ref.Lizard_compress(block.ctypes.data, dst, block.size, cap, level)
        total += c if 0 < c < block.size else block.size
    return total


def ratios(ref, raw, E, levels=LEVELS):
    """{level: {"bytes": ratio, "bits": ratio}} for the bytes `raw` of elements of E bytes."""
    by, bt = pi.split_model(raw, E), bi.bits_split_model(raw, E)
    assert np.array_equal(pi.join_model(by, E), raw) and np.array_equal(bi.bits_join_model(bt, E), raw)
    return {level: {"bytes": round(stored_bytes(ref, by, level) / raw.size, 4), "bits": round(stored_bytes(ref, bt, level) / raw.size, 4)}
            for level in levels}


def inputs():
    """[(name, uint8 array, element size)], generated on the CPU."""
    import torch

    def u8(t):
        return t.contiguous().reshape(-1).view(torch.uint8).numpy()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = torch.randn(2 ** 19) * 0.02
        torch.manual_seed(1)
        a = torch.randn(2 ** 19) * 1.0
        torch.manual_seed(1)
        idx = torch.randint(0, 50000, (2 ** 18,), dtype=torch.int32)
    return [("fp16 randn * 0.02", u8(w.to(torch.float16)), 2), ("bf16 randn * 0.02", u8(w.to(torch.bfloat16)), 2),
            ("fp32 randn * 0.02", u8(w), 4), ("bf16 randn * 1.0", u8(a.to(torch.bfloat16)), 2),
            ("int32 indices < 50000", u8(idx), 4), ("int64 arange(2^17)", u8(torch.arange(2 ** 17, dtype=torch.int64)), 8),
            ("bf16 randn * 0.02, 8 KiB", u8(w[:4096].to(torch.bfloat16)), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitplanes_ratio.json"))
    args = ap.parse_args()
    ref = util.reference()
    if ref is None:
        sys.exit("oracle/_ref/liblizard_ref_reset.so is not present: build the oracle where the reference's sources are")
    res = {"block_bytes": BLOCK, "levels": list(LEVELS), "generator": "torch.manual_seed(1), CPU", "rows": []}
    for name, raw, E in inputs():
        r = ratios(ref, raw, E)
        res["rows"].append({"data": name, "raw_bytes": int(raw.size), "elem_size": E, "ratio": {str(k): v for k, v in r.items()}})
        print("%-26s" % name, "  ".join("L%d %.4f / %.4f" % (k, v["bytes"], v["bits"]) for k, v in r.items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
