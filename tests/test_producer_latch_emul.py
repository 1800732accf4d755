"""CPU: the inputs of tests/producer_latch_inputs.py through the producer / consumer form of levels 10 / 30 on the SIMT emulator
(lizard_amd/csrc/lz_split.h), byte for byte against the oracle, and the emulator's LZ_STAT marks must show that the inputs built for
a path took it.  The emulator's producer is the level-10 instantiation of lz_parse_fast (LANEFORMS: the chain pass with the
lane-prepared backward length and the folded exits) at BOTH levels; the levels differ in the consumer (level 30 entropy-codes the
streams).  The form the level-30 kernel keeps on the device (lz_back_from, the unfolded exits) is not run here: only
tests/test_producer_latch_gpu.py at level 30 runs it."""
import ctypes

import pytest

import producer_latch_inputs as inputs
import util
from test_producer_round_emul import emul_split

MARKS = (8, 9, 10, 11, 12)       # lz_parse_fast: third chained sequence, stale stop, (earlier pass), l1 > 63, fourth round


def _marks(reset=True):
    out = (ctypes.c_ulonglong * 64)()
    util.emulator().emul_stats(out, 1 if reset else 0)
    return {k: int(out[k]) for k in MARKS}


def _run(name, level, seed=1):
    data = dict(inputs.all_blocks())[name]
    _marks()
    assert emul_split(data, len(data), level, nprod=1, ncons=1, seed=seed) == [inputs.expected(level)[name]], (level, name)
    return _marks()


def test_oracle_alone_gives_the_sequences_every_input_aims_for():
    """Flags and literals stream sizes of the oracle's output are exactly those of the sequences (position, length) each builder
    wrote down — backward lengths included — at both levels; the matrix of backward cases is complete."""
    cases = set()
    for name, data, seqs, part in inputs.back_blocks():
        assert inputs._exact(data, seqs), name
        assert 2048 <= len(data) <= 16384, (name, len(data))
        cases |= set(part)
    assert cases == {(t, r, c) for c in (False, True) for t in inputs.BACK_T for r in inputs.BACK_R}
    assert (8, 9, True) in cases                                     # 8 equal bytes with room beyond: the unresolved case
    low = set()
    for name, data, seqs, (M, t) in inputs.low_blocks():
        # the last sequence is X found with candidate M, t bytes longer backwards: the oracle's streams have exactly its sizes
        assert inputs._exact(data, seqs), name
        P, ml = seqs[-1]
        assert ml == 10 + t and data[M - t:M + 10] == data[P:P + ml] and (t == M or data[M - t - 1] != data[P - 1]), name
        assert 2048 <= len(data) <= 16384, (name, len(data))
        low.add((M, t))
    assert low == {(M, t) for M in range(10) for t in range(9) if t <= M}
    assert (8, 8) in low                                             # where lz_back_lane ("open") and lz_back_from (exact) differ
    for name, data, seqs in inputs.chain_blocks():
        assert seqs is None or inputs._exact(data, seqs), name
        assert 1900 <= len(data) <= 16384, (name, len(data))
    sizes = {name: len(data) for name, data in inputs.all_blocks()}
    assert [sizes["tiny%d" % n] for n in inputs.TINY] == list(inputs.TINY)
    assert sizes["two_subblocks9000"] == 131072 + 9000
    for level in inputs.LEVELS:
        assert inputs.stream_sizes(inputs.expected(level)["two_subblocks9000"]) != [None, None]


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_every_input_byte_for_byte(level):
    want = inputs.expected(level)
    for case, (name, data) in enumerate(inputs.all_blocks()):
        assert emul_split(data, len(data), level, nprod=1, ncons=1, seed=case + 1) == [want[name]], (level, name)


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_paths_are_taken(level):
    """The l1 inputs: two 5-byte words, then an 8-byte word that ends in lane l1 with another right behind it.  l1 = 63: the word is
    the round's third chained sequence (mark 8) and the one behind it, in lane 63, leaves through the l1 > 63 exit (mark 11); l1 = 64
    and 65: the word itself leaves through that exit and no third sequence is chained.  The small-alphabet input stops chains at a stale
    reader (mark 9); a run of four rounds without a winner announces its fourth round (mark 12, one more than the input with one such round has) and still finds its word; the chained
    backward cases are not stopped by a stale reader, so their second winner is taken inside the chain pass."""
    for l1, third in ((63, 1), (64, 0), (65, 0)):
        got = _run("l1_%d" % l1, level)
        assert got[8] == third and got[11] == 1 and got[9] == 0, (level, l1, got)
    assert _run("stale_reader", level)[9] > 0
    # (every input opens with 900 literals in front of its first match: one run of four and more rounds, one mark, in each)
    assert _run("winner_nowinner_winner", level)[12] == 1
    assert _run("four_rounds_then_winner", level)[12] == 2
    # (the next two are decided by their bytes: a pass that chained in a later round would go from a to c and lose b, one that chained
    #  on an unresolved backward length would push it as it stands; the marks only say that no pass left through the l1 exit)
    got = _run("second_round_pair", level)
    assert got[11] == 0 and got[8] == 0
    got = _run("unresolved_then_word", level)
    assert got[11] == 0 and got[8] == 0 and got[9] == 0
    for name, _, _, part in inputs.back_blocks():
        if all(c for _, _, c in part):
            got = _run(name, level)
            assert got[9] == 0 and got[11] == 0, (level, name, got)


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_two_producers_share_the_small_inputs(level):
    """The 2 KiB inputs cut to one size as one batch over two producers: what a producer carries from round to round (positions,
    validity mask, lane table) is set up anew for every block."""
    blocks = [d[:1900] for name, d in inputs.all_blocks() if 1900 <= len(d) <= 2700]
    outs = emul_split(b"".join(blocks), 1900, level, nprod=2, ncons=1, seed=11)
    for b, o in zip(blocks, outs):
        assert o == util.oracle_compress(b, level), level
