"""GPU: the blocks of tests/producer_chain_inputs.py through LizardGPU_compressBlocks_device at levels 10, 30, 11 and 31, sizes and
bytes against the oracle: once as ragged launches (the input plus a third of it as the short last block), once as one uniform launch
of 64 blocks per size."""
import pytest

import producer_chain_inputs as inputs
import util
from test_producer_round_gpu import _device_batch

pytestmark = pytest.mark.gpu

UNIFORM_SIZES = (4096, 33 * 1024, 131072 + 13)


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_ragged_batches(level):
    want = inputs.expected(level)
    for name, data in inputs.all_blocks():
        tail = data[:len(data) // 3]
        outs = _device_batch(data + tail, len(data), level)
        assert len(outs) == 2 and outs[0] == want[name], (level, name)
        assert outs[1] == util.oracle_compress(tail, level), (level, name, "tail")


@pytest.mark.parametrize("level", inputs.LEVELS)
@pytest.mark.parametrize("size", UNIFORM_SIZES)
def test_uniform_batch_of_64_blocks(level, size):
    """Every input of at least `size` bytes, its last `size` bytes (the end of a block is where the built inputs differ), repeated
    to 64 blocks of one size."""
    blocks = [d[len(d) - size:] for _, d in inputs.all_blocks() if len(d) >= size]
    blocks = [blocks[i % len(blocks)] for i in range(64)]
    cache = {}
    outs = _device_batch(b"".join(blocks), size, level)
    assert len(outs) == 64
    for i, (b, o) in enumerate(zip(blocks, outs)):
        if b not in cache:
            cache[b] = util.oracle_compress(b, level)
        assert o == cache[b], (level, size, i)
