"""CPU: the inputs of tests/producer_chain_inputs.py through the SIMT emulator, byte for byte against the oracle — the producer /
consumer form of levels 10 / 30 and the one-wave form of levels 11 / 31 (both run lz_parse_fast, lizard_amd/csrc/lz_block.h) — and
the emulator's LZ_STAT counters must show that the paths the inputs were built for were taken."""
import ctypes

import pytest

import producer_chain_inputs as inputs
import util
from test_emulator import emul_compress
from test_producer_round_emul import emul_split

# LZ_STAT marks of lz_parse_fast
REQUIRED = {8: "a third chained sequence out of one round", 9: "a stale reader stops the chain",
            10: "a stale stop caused by an earlier pass's interval", 11: "the chain leaves because l1 > 63",
            12: "a run of four or more rounds"}


def _stats(reset):
    out = (ctypes.c_ulonglong * 64)()
    util.emulator().emul_stats(out, 1 if reset else 0)
    return {k: int(out[k]) for k in REQUIRED}


def test_no_input_is_stored_raw():
    inputs.assert_all_compressed()


def test_boundary_inputs_decide_the_output():
    """Oracle alone: at p + step == mflimit the word is found, at mflimit + 1 it is not (so a wrong `<=` in the schedule shows)."""
    inputs.assert_boundary_decides()


@pytest.mark.parametrize("level", inputs.SPLIT_LEVELS)
def test_split_form_and_its_paths(level):
    """Levels 10 / 30 (LDS exchange table: the per-reader form of the chain loop, the schedule as a recurrence)."""
    _stats(True)
    want = inputs.expected(level)
    for size in inputs.GEN_SIZES:
        blocks = inputs.generated(size)
        outs = emul_split(b"".join(blocks), size, level, nprod=2, ncons=1, seed=size)
        for i, o in enumerate(outs):
            assert o == want["gen%d_s%d" % (size, 8 + i)], (level, size, i)
    for case, (name, data) in enumerate(inputs.built()):
        assert emul_split(data, len(data), level, nprod=1, ncons=1, seed=case + 1) == [want[name]], (level, name)
    got = _stats(True)
    missing = [v for k, v in REQUIRED.items() if got[k] == 0]
    assert not missing, (missing, got)


@pytest.mark.parametrize("level", (10, 30, 11, 31))
def test_one_wave_form_and_its_paths(level):
    """The instantiations that keep the mask form of the chain loop and the general schedule.  Levels 10 / 30 as one wave per block:
    the exchange-table form the level-30 kernel runs on the device (and, on odd emulator seeds, the plain global-memory table); every
    mark must be reached.  Levels 11 / 31 (global-memory table with tag de-duplication, narrow first rounds: the mask form of the chain loop and the general
    schedule), with and without the occupancy summary.  Only a run's first round chains and there it is 32 slots wide: a winner in
    lane <= 31 with a length the batch resolves (<= 24) ends in lane <= 55, so the l1 > 63 exit cannot be reached at these levels;
    every other mark must be.  (This rests on LZ_WIDE_W0 = 32 in lz_block.h: with first rounds of 64 slots the exit is reachable and
    the `== 0` below fails, which is the reminder to require it here too.)"""
    _stats(True)
    want = inputs.expected(level)
    for case, (name, data) in enumerate(inputs.all_blocks()):
        assert emul_compress(data, level, seed=case + 1) == want[name], (level, name)
    got = _stats(True)
    narrow = level in (11, 31)
    missing = [v for k, v in REQUIRED.items() if got[k] == 0 and not (narrow and k == 11)]
    assert not missing and not (narrow and got[11]), (missing, got)
