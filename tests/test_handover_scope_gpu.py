"""GPU: the hand-over of sequence buffers between the producer and consumer waves of levels 10 / 30 (lizard_amd/csrc/lz_split.h) with
its fences at workgroup scope (lz_publish_release / lz_publish_acquire, lz_wave.h): a consumer must read the list its producer wrote
into a buffer NOW, not what the buffer held in an earlier use.  16 distinct blocks, so neighbouring uses of a buffer hold different
lists; every output is compared with the oracle's answer for its distinct block, computed once each.

  test_three_jobs_per_block   blocks of 2 x 131 072 + 4 096 bytes: three jobs per block through two buffers (the third job refills the
                              first buffer; the last sub-block is short), 2 080 blocks in one launch, then 8 blocks in a second launch
                              (fewer blocks than CUs: one active producer per workgroup).
  test_many_jobs_per_producer blocks of 4 096 bytes, 32 for each producer of a full launch (13 x 256 x 32): a launch with at least as
                              many blocks as producers runs every producer until the block counter is used up, and each refills
                              its two buffers about sixteen times each."""
import functools

import pytest

from test_producer_round_gpu import _device_batch
import util

pytestmark = pytest.mark.gpu

LEVELS = (10, 30)
BIG = 2 * 131072 + 4096
SMALL = 4096


@functools.lru_cache(maxsize=None)
def distinct(size):
    return tuple(util.datagen(size, 0.3 + 0.03 * seed, 0.0, 400 + seed) for seed in range(16))


@functools.lru_cache(maxsize=None)
def expected(size, level):
    return tuple(util.oracle_compress(b, level) for b in distinct(size))


def check_rotation(size, n, level):
    blocks, want = distinct(size), expected(size, level)
    assert len(set(blocks)) == 16 and len(set(want)) == 16
    outs = _device_batch(b"".join(blocks[i % 16] for i in range(n)), size, level)
    assert len(outs) == n
    bad = [i for i, o in enumerate(outs) if o != want[i % 16]]
    assert not bad, (level, size, n, len(bad), bad[:8])


@pytest.mark.parametrize("level", LEVELS)
def test_three_jobs_per_block(level):
    check_rotation(BIG, 2080, level)
    check_rotation(BIG, 8, level)


@pytest.mark.parametrize("level", LEVELS)
def test_many_jobs_per_producer(level):
    check_rotation(SMALL, 13 * 256 * 32, level)
