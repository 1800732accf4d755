"""CPU: what the XOR-with-base filter is for, measured with the unmodified reference library (util.reference(): oracle/_ref, built with
-DLIZARD_RESET_MEM) on the numpy model of the byte-plane layout applied to tensor XOR base.  torch.manual_seed(1);
w = randn(2^19) * 0.02; step = 1e-5 * sign(randn) * rand from the same generator; the tensor is w + step, the base w, both cast to
bf16, fp16 and fp32; split whole, compressed in 128 KiB blocks with Lizard_compress, a block counting with its own size when it does
not shrink; stream / raw.  At level 10 the reference gives 0.3090 / 0.4935 / 0.6608 with XOR + byte planes against 0.8430 / 1.0000 /
0.9215 with byte planes alone (scripts/xor_base_ratio.py, profiles/xor_base_ratio.json); the bounds below — 0.40 / 0.60 / 0.75 —
leave room for another torch generator only.  And the documented loss stays true: bf16 against an UNRELATED base (randn * 0.02 under
manual_seed(2)) at level 10 is larger with XOR + byte planes than without."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util
import planes_inputs as pi

BLOCK = 128 << 10
N = 2 ** 19


@pytest.fixture(scope="module")
def ref():
    R = util.reference()
    if R is None:
        util.need_ref("oracle/_ref/liblizard_ref_reset.so")
    return R


def stored(R, data, level):
    cap = R.Lizard_compressBound(BLOCK)
    dst = C.create_string_buffer(cap)
    total = 0
    for at in range(0, data.size, BLOCK):
        block = np.ascontiguousarray(data[at:at + BLOCK])
        c = R.Lizard_compress(block.ctypes.data, dst, block.size, cap, level)
        assert c > 0
        total += min(c, block.size)
    return total


def both(R, t, b, level):
    """(byte planes alone, XOR with b + byte planes) of tensor t: stream / raw."""
    import torch
    E = t.element_size()
    raw, base = t.contiguous().view(torch.uint8).numpy(), b.contiguous().view(torch.uint8).numpy()
    plain, xored = pi.split_model(raw, E), pi.split_model(raw ^ base, E)
    assert np.array_equal(pi.join_model(xored, E) ^ base, raw)
    return stored(R, plain, level) / raw.size, stored(R, xored, level) / raw.size


def test_a_small_step_behind_the_base_shrinks_at_level_10(ref):
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = torch.randn(N) * 0.02
        step = 1e-5 * torch.sign(torch.randn(N)) * torch.rand(N)
    for name, dt, bound in (("bf16", torch.bfloat16, 0.40), ("fp16", torch.float16, 0.60), ("fp32", torch.float32, 0.75)):
        plain, xored = both(ref, (w + step).to(dt), w.to(dt), 10)
        print("%s lr 1e-5, level 10: byte planes %.4f, XOR + byte planes %.4f" % (name, plain, xored))
        assert xored < plain, (name, plain, xored)
        assert xored < bound, (name, xored)


def test_an_unrelated_base_loses_at_level_10_with_byte_planes(ref):
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        w = torch.randn(N) * 0.02
        torch.manual_seed(2)
        other = torch.randn(N) * 0.02
    plain, xored = both(ref, w.to(torch.bfloat16), other.to(torch.bfloat16), 10)
    print("bf16 against an unrelated base, level 10: byte planes %.4f, XOR + byte planes %.4f" % (plain, xored))
    assert xored > plain, (plain, xored)
