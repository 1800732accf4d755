"""GPU: the blocks of tests/count_trip_inputs.py through LizardGPU_compressBlocks_device at levels 10 and 30, sizes and bytes against
the oracle: every input as a ragged launch (the input plus its first third as the short last block) and as one uniform launch of 64
blocks.  Level 10 runs the late back trip (lz_block.h), level 30 the two count calls in a row."""
import pytest

import count_trip_inputs as inputs
import util

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_ragged_pairs(level):
    want = inputs.expected(level)
    for name, data in inputs.all_blocks():
        tail = data[:max(1, len(data) // 3)]
        outs = inputs.device_batch(data + tail, len(data), level)
        assert len(outs) == 2 and outs[0] == want[name], (level, name)
        assert outs[1] == util.oracle_compress(tail, level), (level, name, "tail")


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_uniform_launches_of_64_blocks(level):
    """The input 64 times in one launch: every producer of several workgroups takes it with whatever it carried before."""
    want = inputs.expected(level)
    for name, data in inputs.all_blocks():
        outs = inputs.device_batch(data * 64, len(data), level)
        assert len(outs) == 64
        assert all(o == want[name] for o in outs), (level, name, [i for i, o in enumerate(outs) if o != want[name]][:4])
