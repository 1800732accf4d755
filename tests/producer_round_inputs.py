"""Inputs of tests/test_producer_round_emul.py and tests/test_producer_round_gpu.py: blocks of 4-131 KiB chosen to walk the paths
of the producers' parse loop (lizard_amd/csrc/lz_block.h, lz_parse_fast): rounds with and without a winner, chained winners,
the make-up sweeps behind a long match, runs that reach mflimit, winners without a backward fetch, the sub-block hand-over."""
import functools
import random

import util

LEVELS = (10, 30)
GEN_SIZES = (4096, 33 * 1024, 65536 + 5)        # 33 KiB: one sweep boundary of the 17-bit table (every 32 768 positions) crossed


@functools.lru_cache(maxsize=None)
def generated(size):
    """datagen P50, seeds 0-7."""
    return tuple(util.datagen(size, 0.5, 0.0, seed) for seed in range(8))


def _edges_case():
    """A compressible block whose first bytes come back later (the candidate lies in the first 8 bytes: nothing to fetch behind it,
    haveBack is false) and whose last match runs into the end (it is cut at matchlimit, inside LZ_MFLIMIT of the sub-block's end)."""
    n = 20000
    b = bytearray(util.datagen(n, 0.5, 0.0, 77))
    b[0:16] = bytes(range(200, 216))             # sixteen bytes found nowhere else ...
    b[300:316] = b[0:16]                         # ... until position 300: its candidate is position 0
    b[900:914] = b[2:16]                         # candidate at position 2, one byte of backward room at most
    b[n - 70:n] = b[5000:5070]                   # a match that would reach the last byte
    return bytes(b)


@functools.lru_cache(maxsize=None)
def special():
    """(name, data, compressible) — compressible: the oracle must store it as a compressed block (True) or raw (False)."""
    return (
        ("one_byte", b"\x5a" * 65536, True),                       # one long match: make-up sweeps, a chain that stops at lane 63
        ("period2", b"ab" * 32768, True),
        ("noise", random.Random(5).randbytes(48 * 1024), False),   # no round has a winner, every run ends at mflimit
        ("edges", _edges_case(), True),
        ("two_subblocks", util.datagen(131072 + 13, 0.5, 0.0, 9), True),   # hand-over, the `special` reset, two job headers
    )


def all_blocks():
    # (a 4 KiB block has to save the 512 bytes the container asks of a compressed sub-block: some seeds do, some are stored raw — None)
    out = [("gen%d_s%d" % (size, seed), d, True if size > 4096 else None) for size in GEN_SIZES for seed, d in enumerate(generated(size))]
    return out + list(special())


@functools.lru_cache(maxsize=None)
def expected(level):
    """name -> the oracle's output; computed once per level and shared."""
    return {name: util.oracle_compress(data, level) for name, data, _ in all_blocks()}
