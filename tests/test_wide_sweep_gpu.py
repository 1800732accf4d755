"""GPU: the sweep_* blocks of tests/producer_tail_inputs.py (decisions that hang on a table sweep: a word 65 535 back is found, the
same word 65 536 back is not; entries 2^17 + 100 old with the same bytes and check bits) and the block of 131 072 + 9 000 bytes whose
second sub-block starts with a sweep due, through LizardGPU_compressBlocks_device at levels 10 and 30, sizes and bytes against the
oracle.  Each block runs as a ragged pair (the block and its first third) and 64 times in one launch: 13 (12) producers of several
workgroups sweep tables that start 8-aligned and 4 bytes off."""
import functools

import pytest

import producer_tail_inputs as inputs
from test_producer_round_gpu import _device_batch
import util

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def blocks():
    out = tuple((name, data) for name, data in inputs.all_blocks() if name.startswith("sweep_") or name == "two_subblocks9000")
    assert len(out) == 8 and len(dict(out)["two_subblocks9000"]) == 131072 + 9000
    return out


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_ragged_pairs(level):
    want = inputs.expected(level)
    for name, data in blocks():
        tail = data[:len(data) // 3]
        outs = _device_batch(data + tail, len(data), level)
        assert len(outs) == 2 and outs[0] == want[name], (level, name)
        assert outs[1] == util.oracle_compress(tail, level), (level, name, "tail")


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_64_blocks_in_one_launch(level):
    want = inputs.expected(level)
    for name, data in blocks():
        outs = _device_batch(data * 64, len(data), level)
        assert len(outs) == 64
        assert all(o == want[name] for o in outs), (level, name, [i for i, o in enumerate(outs) if o != want[name]][:4])
