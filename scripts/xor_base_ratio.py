#!/usr/bin/env python3
"""What the XOR-with-base filter (include/lizard_amd.h Part 3c) gains in front of the byte-plane and the bit-plane filter, and where it
loses, on the CPU, without a GPU: the numpy models of both layouts (tests/planes_inputs.py, tests/bitplanes_inputs.py) applied to
tensor XOR base, and the unmodified reference library under oracle/_ref (built with -DLIZARD_RESET_MEM, tests/util.py).  Every input
is split whole, cut into 128 KiB blocks, each block through Lizard_compress; a block counts with its compressed size when that is
below its own size and with its own size otherwise (what a frame stores); the sum over raw bytes is the ratio.
Inputs (inputs() below): torch.manual_seed(1); w = randn(2^19) * 0.02; from the same generator step = lr * sign(randn) * rand, an
Adam-sized update with |step| <= lr; the tensor is w + step, the base w, both cast to the dtype — bf16, fp16 and fp32 at lr 1e-5,
bf16 at lr 1e-4 and 1e-3; bf16 with 1 % of the elements replaced by new values; and bf16 w against an UNRELATED base
(randn * 0.02 under manual_seed(2)), the row where the filter loses.  Levels 10, 21, 30, 41.  Writes profiles/xor_base_ratio.json.

    python scripts/xor_base_ratio.py [--out profiles/xor_base_ratio.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bitplanes_inputs as bi
import planes_inputs as pi
import util
from bitplanes_ratio import BLOCK, LEVELS, stored_bytes

N = 2 ** 19
KINDS = ("bytes", "xor_bytes", "bits", "xor_bits")


def ratios(ref, raw, base, E, levels=LEVELS):
    """{level: {"bytes", "xor_bytes", "bits", "xor_bits": ratio}} for the bytes `raw` of elements of E bytes and their base."""
    x = raw ^ base
    split = {"bytes": pi.split_model(raw, E), "xor_bytes": pi.split_model(x, E), "bits": bi.bits_split_model(raw, E),
             "xor_bits": bi.bits_split_model(x, E)}
    assert np.array_equal(pi.join_model(split["xor_bytes"], E) ^ base, raw) and np.array_equal(bi.bits_join_model(split["xor_bits"], E) ^ base, raw)
    return {level: {k: round(stored_bytes(ref, split[k], level) / raw.size, 4) for k in KINDS} for level in levels}


def u8(t):
    import torch
    return t.contiguous().reshape(-1).view(torch.uint8).numpy()


def stepped(lr):
    """(w + step, w) as fp32, from torch.manual_seed(1)."""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = torch.randn(N) * 0.02
        step = lr * torch.sign(torch.randn(N)) * torch.rand(N)
    return w + step, w


def replaced(share):
    """(w with `share` of its elements replaced by new values, w) as fp32, from torch.manual_seed(1)."""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = torch.randn(N) * 0.02
        hit = torch.rand(N) < share
        new = torch.randn(N) * 0.02
    return torch.where(hit, new, w), w


def unrelated():
    """(w from torch.manual_seed(1), another randn * 0.02 from torch.manual_seed(2)) as fp32."""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = torch.randn(N) * 0.02
        torch.manual_seed(2)
        other = torch.randn(N) * 0.02
    return w, other


def inputs():
    """[(name, tensor bytes, base bytes, element size, share of elements that differ)], generated on the CPU."""
    import torch
    rows = []
    for name, (t, b), dt in (("bf16, lr 1e-5", stepped(1e-5), torch.bfloat16), ("fp16, lr 1e-5", stepped(1e-5), torch.float16),
                             ("fp32, lr 1e-5", stepped(1e-5), torch.float32), ("bf16, lr 1e-4", stepped(1e-4), torch.bfloat16),
                             ("bf16, lr 1e-3", stepped(1e-3), torch.bfloat16), ("bf16, 1 % of elements replaced", replaced(0.01), torch.bfloat16),
                             ("bf16, UNRELATED base", unrelated(), torch.bfloat16)):
        t, b = t.to(dt), b.to(dt)
        E = t.element_size()
        differ = float((u8(t).reshape(-1, E) != u8(b).reshape(-1, E)).any(axis=1).mean())
        rows.append((name, u8(t), u8(b), E, differ))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xor_base_ratio.json"))
    args = ap.parse_args()
    ref = util.reference()
    if ref is None:
        sys.exit("oracle/_ref/liblizard_ref_reset.so is not present: build the oracle where the reference's sources are")
    res = {"block_bytes": BLOCK, "levels": list(LEVELS), "generator": "torch.manual_seed(1), CPU; the unrelated base manual_seed(2)",
           "columns": list(KINDS), "rows": []}
    for name, raw, base, E, differ in inputs():
        r = ratios(ref, raw, base, E)
        res["rows"].append({"data": name, "raw_bytes": int(raw.size), "elem_size": E, "elements_that_differ": round(differ, 4),
                            "ratio": {str(k): v for k, v in r.items()}})
        print("%-32s %5.1f %% differ " % (name, 100 * differ),
              "  ".join("L%d %s" % (k, " / ".join("%.4f" % v[c] for c in KINDS)) for k, v in r.items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
