"""GPU: the blocks of tests/producer_round_inputs.py through LizardGPU_compressBlocks_device at levels 10 and 30, sizes and bytes
against the oracle.  The device entry takes ONE block size and a shorter last block, so the ragged form is a launch per input with
a third of the input again as its short last block; the uniform form is a launch of 64 equal blocks per size."""
import numpy as np
import pytest

import producer_round_inputs as inputs
import util

pytestmark = pytest.mark.gpu


def _device_batch(data, bs, level):
    import torch
    from lizard_amd import api
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    dst, sizes, stride = api.compress_blocks_device(src, bs, level)
    torch.cuda.synchronize()
    out, sz = dst.cpu().numpy(), sizes.cpu().numpy()
    return [out[i * stride:i * stride + int(sz[i])].tobytes() for i in range(len(sz))]


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_ragged_batches(level):
    want = inputs.expected(level)
    for name, data, _ in inputs.all_blocks():
        tail = data[:len(data) // 3]
        outs = _device_batch(data + tail, len(data), level)
        assert len(outs) == 2 and outs[0] == want[name], (level, name)
        assert outs[1] == util.oracle_compress(tail, level), (level, name, "tail")


@pytest.mark.parametrize("level", inputs.LEVELS)
@pytest.mark.parametrize("size", inputs.GEN_SIZES)
def test_uniform_batch_of_64_blocks(level, size):
    """Eight generated blocks and every special block's first `size` bytes, repeated to 64 blocks of one size."""
    blocks = list(inputs.generated(size)) + [d[:size] for _, d, _ in inputs.special() if len(d) >= size]
    blocks = [blocks[i % len(blocks)] for i in range(64)]
    cache = {}
    outs = _device_batch(b"".join(blocks), size, level)
    assert len(outs) == 64
    for i, (b, o) in enumerate(zip(blocks, outs)):
        if b not in cache:
            cache[b] = util.oracle_compress(b, level)
        assert o == cache[b], (level, size, i)
