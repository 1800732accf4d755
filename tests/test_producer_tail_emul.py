"""CPU: the inputs of tests/producer_tail_inputs.py through the producer / consumer form of levels 10 / 30 on the SIMT emulator
(lizard_amd/csrc/lz_split.h; level 10 keeps the sequence list's tail in lanes and tests for sweeps where lane 0 moves on, level 30
keeps the LDS ring and the test at the head of the round), sizes and bytes against the oracle."""
import ctypes

import pytest

import producer_tail_inputs as inputs
import util
from test_producer_round_emul import emul_split


def _marks(reset):
    out = (ctypes.c_ulonglong * 64)()
    util.emulator().emul_stats(out, 1 if reset else 0)
    return {k: int(out[k]) for k in (8, 9)}


def test_inputs_have_the_sequence_counts_they_aim_for():
    """Oracle alone (the builders assert while they search their seeds; this is the finished list): every count, both ends, no
    sub-block stored raw except the 13-byte one, blocks of the sizes asked for."""
    seen = set()
    for name, data, want in inputs.built():
        for level in inputs.LEVELS:
            got = inputs.seq_counts(inputs.expected(level)[name])
            assert want is None or got == want, (name, level, got, want)
            assert None not in got or name == "two_subblocks13", (name, level, got)
        if name.startswith(("count", "dense")):
            assert 2048 <= len(data) <= 16384, (name, len(data))
            seen.add(want[0])
        if name.startswith("sweep"):
            assert 70 * 1024 <= len(data) <= 140 * 1024, (name, len(data))
    assert seen == set(inputs.COUNTS)
    assert len(dict(inputs.all_blocks())["two_subblocks13"]) == 131072 + 13


def test_chain_model_places_the_64th_and_128th_push_inside_the_chain_loop():
    """The inputs alone: by the model of a round (chain_model) push 64, and push 128 where there is a 129th sequence, is made inside
    the chain loop in every chained input that has that many."""
    for name, data, seqs, count in inputs.dense_cases():
        inside, _ = inputs.chain_model(seqs, len(data))
        assert count < 65 or 64 in inside, name
        assert count < 129 or 128 in inside, name


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_chained_rounds_across_the_wrap(level):
    """Copies 4-6 literals apart: the rounds chain, and pushes 64 and 128 are among the chained ones.  The model that says so is
    checked against the emulator's marks: as many rounds with a third chained sequence as it predicts (mark 8), and no chain stopped
    by a stale reader (mark 9), which the model does not know."""
    want = inputs.expected(level)
    for case, (name, data, seqs, count) in enumerate(inputs.dense_cases()):
        _marks(True)
        assert emul_split(data, len(data), level, nprod=1, ncons=1, seed=case + 1) == [want[name]], (level, name)
        got = _marks(True)
        inside, rounds3 = inputs.chain_model(seqs, len(data))
        assert got[9] == 0 and got[8] == rounds3, (level, name, got, rounds3)


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_every_input_byte_for_byte(level):
    want = inputs.expected(level)
    for case, (name, data) in enumerate(inputs.all_blocks()):
        assert emul_split(data, len(data), level, nprod=1, ncons=1, seed=case + 1) == [want[name]], (level, name)


@pytest.mark.parametrize("level", inputs.LEVELS)
def test_two_producers_share_the_small_inputs(level):
    """The count inputs cut to one size and run as one batch over two producers: a producer's lane table is emptied at the end of every
    sub-block, whatever the block before left in it."""
    blocks = [d[:2048] for name, d in inputs.all_blocks() if name.startswith(("count", "dense"))]
    outs = emul_split(b"".join(blocks), 2048, level, nprod=2, ncons=1, seed=7)
    for b, o in zip(blocks, outs):
        assert o == util.oracle_compress(b, level), level
