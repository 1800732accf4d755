"""CPU: the chain build of the hashChain / noChain levels (lz_hc_begin, lz_hc_build, lz_hc_hits_plain / lz_hc_hits of
lizard_amd/csrc/lz_hashchain.h) on the SIMT emulator, table by table against the sequential model exported from the oracle
(lzo_hc_tables, oracle/lizard_oracle.h) over the named inputs of tests/hc_build_inputs.py — and which paths of the build those inputs
reach (the LZ_HC_MARK marks of lz_hc_build).  tests/test_hc_build_gpu.py runs the same inputs through the same functions on the device,
where nothing can count marks: that the set is worth running there is established here."""
import ctypes

import numpy as np
import pytest

import hc_build_inputs as H
import util

_c = ctypes
BEST_OPEN = 0xFFFFFFFF


def _emulator():
    E = util.emulator()
    E.emul_hc_tables.argtypes = [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int] + [_c.c_void_p] * 4 + [_c.c_uint]
    E.emul_hc_tables.restype = _c.c_int
    E.emul_hc_marks.argtypes = [_c.c_void_p, _c.c_int, _c.c_int]
    E.emul_hc_marks.restype = None
    return E


@pytest.fixture(scope="module")
def models():
    """(case index, oracle level) -> the model's tables as numpy arrays, computed once."""
    out = {}
    for ci, vi in H.jobs():
        level, pre = H.VARIANTS[vi][5], H.VARIANTS[vi][4]
        if (ci, level) not in out:
            t = util.oracle_hc_tables(H.cases()[ci][1], level, with_first=bool(pre))
            out[(ci, level)] = {k: np.array(v, dtype=np.uint32) for k, v in t.items()}
    return out


def run_tables(E, data, variant, seed):
    _, sl, hl, sn, pre, _, _ = variant
    n = len(data)
    n_ins = n - 7 if n >= 8 else 0
    words = (n_ins + 63) // 64
    src = _c.create_string_buffer(data, n) if n else _c.create_string_buffer(1)
    prev, chain2 = np.zeros(max(n_ins, 1), np.uint16), np.zeros(max(n_ins, 1), np.uint32)
    hits, best = np.zeros(max(words, 1), np.uint64), np.zeros(max(n_ins, 1), np.uint32)
    r = E.emul_hc_tables(src, n, sl, hl, sn, pre, prev.ctypes.data, chain2.ctypes.data, hits.ctypes.data, best.ctypes.data, seed)
    assert r == 0, ("canary or pool mask", r)
    assert src.raw[:n] == data
    return prev[:n_ins], chain2[:n_ins], hits[:words], best[:n_ins]


def check_tables(name, n_ins, got, model, pre):
    """The rules both harnesses apply; returns the number of decided positions."""
    prev, chain2, hits, best = got
    assert np.array_equal(prev, model["prev"]), (name, "prev", int(np.argmax(prev != model["prev"])))
    assert np.array_equal(chain2, model["two"]), (name, "chain2", int(np.argmax(chain2 != model["two"])))
    bits = np.unpackbits(hits.view(np.uint8), bitorder="little")
    assert np.array_equal(bits[:n_ins], model["hit"]), (name, "hits", int(np.argmax(bits[:n_ins] != model["hit"])))
    assert not bits[n_ins:].any(), (name, "hit bits at and beyond nIns in the last written word")
    if not pre:
        return 0
    is_open = best == BEST_OPEN
    assert not (is_open & (model["mayBeOpen"] == 0)).any(), (name, "open where the model decides", int(np.argmax(is_open & (model["mayBeOpen"] == 0))))
    wrong = ~is_open & (best != model["first"])
    assert not wrong.any(), (name, "best", int(np.argmax(wrong)), int(best[np.argmax(wrong)]), int(model["first"][np.argmax(wrong)]))
    return int((~is_open).sum())


@pytest.fixture(scope="module")
def run_all(models):
    """Every job on two scheduling seeds; per case name the marks it reached, and per job the decided / decided non-zero counts."""
    E = _emulator()
    stats = (_c.c_ulonglong * H.MARK_COUNT)()
    E.emul_hc_marks(stats, H.MARK_COUNT, 1)
    reached, decided = {}, {}
    for k, (ci, vi) in enumerate(H.jobs()):
        name, data, _ = H.cases()[ci]
        v = H.VARIANTS[vi]
        model = models[(ci, v[5])]
        n_ins = len(data) - 7 if len(data) >= 8 else 0
        for seed in (2 * k + 1, 2 * k + 2):
            got = run_tables(E, data, v, seed)
            d = check_tables("%s/%s" % (name, v[0]), n_ins, got, model, v[4])
        if v[4]:
            best = got[3]
            decided[(name, v[0])] = (d, int(((best != BEST_OPEN) & (best != 0)).sum()), n_ins)
        E.emul_hc_marks(stats, H.MARK_COUNT, 1)
        reached.setdefault(name, set()).update(i for i in range(H.MARK_COUNT) if stats[i])
    return reached, decided


def test_every_table_equals_the_model(run_all):
    """prev, chain2 and every hit bit equal the model's for all p < nIns, the hit bits of the last written word beyond nIns are 0,
    best[] is open only where the model allows it and equals the model's first search everywhere else (asserted in the fixture, on
    two lane schedules per job).  A case that contains a repeat has a decided non-zero entry: no pass on an all-open table."""
    reached, decided = run_all
    assert H.total_bytes() <= 8 << 20
    for (name, vname), (d, nz, n_ins) in sorted(decided.items()):
        print("%-32s %-10s decided %7d of %7d, non-zero %6d" % (name, vname, d, n_ins, nz))
    assert sum(1 for _, _, rep in H.cases() if rep) >= 15
    for name, _, rep in H.cases():
        if rep:
            for v in H.VARIANTS:
                if v[4] and (name, v[0]) in decided:
                    assert decided[(name, v[0])][1] >= 1, (name, v[0])


def test_the_set_reaches_every_mark_of_the_build(run_all):
    """Every path of lz_hc_build that has a mark is reached, and by the case that is in the set for it."""
    reached, _ = run_all
    M = H.MARKS
    assert set().union(*reached.values()) == set(M.values())
    assert M["pass3_more_loop"] in reached["const_40k"] and M["scalar_replay"] in reached["const_40k"]
    assert M["scalar_replay"] in reached["period3_40k"] and M["scalar_replay"] in reached["period7_40k"]
    assert M["step_straddles_bins"] in reached["size_1030"]
    assert {M["heads_stored"], M["heads_loaded"]} <= reached["seg_plus_1"]
    assert {M["heads_stored"], M["heads_loaded"]} <= reached["chunk_across_segments"]
    assert {M["bin_left_fresh"], M["heads_loaded"]} <= reached["period9_then_noise"]
    assert not reached["size_0"] and not reached["size_7"]
    for name, data, _ in H.cases():                               # one segment: the head tables never travel
        if len(data) - 7 <= H.SEG:
            assert not ({M["heads_stored"], M["heads_loaded"], M["bin_left_fresh"], M["trailing_bin_fresh"]} & reached[name]), name
