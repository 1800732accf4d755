"""CPU: what the seven check bits of the level-10 table (lizard_amd/csrc/lz_block.h, LzTab::entry, LZ_CHECK_LO) let through, on the
SIMT emulator (tests/emul/count_trip_api.cpp): P50 and P90 data, 256 KiB, seeds 0..3, one producer.

A probe is eligible when its slot's entry passes everything but the bytes (age in [8, 65535], not below lowPos); among the eligible
probes whose four bytes differ from the position's, ideal check bits let 1 in 128 through to the candidate batch, where its 4-byte
test fails.  Asserted: failed 4-byte tests per eligible non-matching probe <= 1.25 / 128 over the four seeds of each kind of data,
and every output the oracle's.  The top seven bits of the same product (LZ_CHECK_LO=25, what the table used before) are measured
beside them and printed; they are nearly a function of the slot index and miss this bound (profiles/count_trip_ab.txt)."""
import pytest

import count_trip_emul as emul
import util

SEEDS = (0, 1, 2, 3)
KINDS = (("P50", 0.5), ("P90", 0.9))
BOUND = 1.25 / 128


@pytest.fixture(scope="module")
def blocks():
    return {(kind, seed): util.datagen(262144, p, 0.0, seed) for kind, p in KINDS for seed in SEEDS}


@pytest.fixture(scope="module")
def oracle_bytes(blocks):
    return {k: util.oracle_compress(d, 10) for k, d in blocks.items()}


def _measure(L, blocks, oracle_bytes, kind):
    """(failed 4-byte tests, eligible non-matching probes, rounds without a winner, those that issued a batch) over the seeds."""
    tot = [0, 0, 0, 0]
    for seed in SEEDS:
        data = blocks[(kind, seed)]
        emul.marks(L)
        out = emul.run(L, data, [(0, len(data))], 10, seed=seed + 1)[0]
        assert out == oracle_bytes[(kind, seed)], (kind, seed)
        m = emul.marks(L)
        print("%s seed %d: failed 4-byte tests %d, eligible non-matching probes %d (1/%.1f); rounds without a winner %d, with a batch %d"
              % (kind, seed, m[4], m[6], m[6] / max(m[4], 1), m[7], m[5]))
        for i, k in enumerate((4, 6, 7, 5)):
            tot[i] += m[k]
    return tot


@pytest.mark.parametrize("kind", [k for k, _ in KINDS])
def test_false_candidates_per_eligible_probe(blocks, oracle_bytes, kind):
    L = emul.lib()
    assert emul.knobs(L)[1] != 25, "the tree builds the table with the top seven bits of the product"
    fail, probes, rounds, batches = _measure(L, blocks, oracle_bytes, kind)
    print("%s, LZ_CHECK_LO=%d: %d / %d = 1/%.1f; %d of %d rounds without a winner issue a batch" % (kind, emul.knobs(L)[1], fail, probes, probes / fail, batches, rounds))
    assert probes > 100000
    assert fail <= BOUND * probes, (kind, fail, probes, "1/%.1f" % (probes / fail))


@pytest.mark.parametrize("kind", [k for k, _ in KINDS])
def test_top_bits_for_comparison(blocks, oracle_bytes, kind):
    """The field the table used before: same bytes out (the check bits never reach the output); its rate is printed, not asserted."""
    L = emul.lib(check_lo=25)
    assert emul.knobs(L)[1] == 25
    fail, probes, rounds, batches = _measure(L, blocks, oracle_bytes, kind)
    print("%s, LZ_CHECK_LO=25: %d / %d = 1/%.1f; %d of %d rounds without a winner issue a batch" % (kind, fail, probes, probes / fail, batches, rounds))
