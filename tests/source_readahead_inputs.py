"""Inputs of tests/test_source_readahead_emul.py and tests/test_source_readahead_gpu.py: the blocks the source read-ahead of the
level-10 producers (lizard_amd/csrc/lz_touch.h) is checked on, and what the oracle makes of them.  Everything is generated from
seeds; the oracle's outputs are computed once per process."""
import functools

import numpy as np

import util

LEVEL = 10                                       # the only level whose producers read ahead (the level-30 kernel keeps the parent's loop)
SIZES = (21, 22, 1023, 1024, 1025, 4096, 131072, 131072 + 13, 131072 + 9000, 262144)
REPEAT_SIZE = 131072 + 9000                      # the 515-byte-period block: two sub-blocks, every match runs to its sub-block's end
# the ragged batch: (bytes in front of the block, block size) — every block starts at an odd address (the area itself is 16-byte
# aligned at least), and the last one ends at the last byte of the area
RAGGED = ((1, 1025), (1, 4109), (3, 21), (1, 131072 + 13), (1, 9001))


@functools.lru_cache(maxsize=None)
def compressible(size):
    return util.datagen(size, 0.5, 0.0, 40 + size % 97)


@functools.lru_cache(maxsize=None)
def incompressible(size):
    return np.random.RandomState(size).randint(0, 256, size, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def repeat515(size=REPEAT_SIZE):
    period = np.random.RandomState(515).randint(0, 256, 515, dtype=np.uint8).tobytes()
    return (period * (size // 515 + 1))[:size]


def all_blocks():
    """(name, bytes, the block's rounds outrun what the read-ahead may ask for per round: see tests/test_source_readahead_emul.py)"""
    out = []
    for n in SIZES:
        out.append(("p50_%d" % n, compressible(n), False))
        out.append(("noise_%d" % n, incompressible(n), n >= 1024))
    out.append(("repeat515_%d" % REPEAT_SIZE, repeat515(), True))
    return out


@functools.lru_cache(maxsize=None)
def ragged_area():
    """(area bytes, [(offset, size)]): P50 data throughout, the blocks of RAGGED cut out of it."""
    total = sum(gap + n for gap, n in RAGGED)
    area = util.datagen(total, 0.5, 0.0, 77)
    at, blocks = 0, []
    for gap, n in RAGGED:
        at += gap
        blocks.append((at, n))
        at += n
    assert at == len(area) and all(o % 2 == 1 for o, _ in blocks)
    return area, blocks


@functools.lru_cache(maxsize=None)
def expected(data):
    return util.oracle_compress(data, LEVEL)
