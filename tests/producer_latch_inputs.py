"""Inputs of tests/test_producer_latch_emul.py and tests/test_producer_latch_gpu.py: blocks of 2-16 KiB (and one of 131 072 + 9 000
bytes) built for the chain pass of the level-10 producers' round (lizard_amd/csrc/lz_block.h, LZ_LATCH_CHAIN) and for what a round
hands to the next: the winner's backward length from what its lane prepared (lz_back_lane), the folded exits of the chain pass, the
rounds whose valid lanes are a proper prefix, both ways out of the loop, and rounds with and without a winner in turn.

How a round lies over the input (tests/producer_chain_inputs.py): behind a match that ends at ip, lane 0 is put(ip - 2), lane 1 the
probe of ip, lane k >= 2 the position ip + k - 1; a run that finds nothing goes on with visits 62.. (producer_tail_inputs.visit_pos).

Backward extension.  A match extends backwards over bytes the table never saw.  Positions a run steps over are not inserted: 514
visits into a run the step is 9, so the 8 bytes in front of a visited position are a window nothing points into.  A window holds
Y (9 bytes) and, at the visited position, X (10 bytes).  Later X comes back behind the last t bytes of Y: it is found at X and
extends backwards over t bytes, or over fewer when the sequence before it ends r < t bytes in front of X.  The same window, with
X standing at position M = 0..9 of the block the first time, gives a candidate in front of which less than 8 bytes can be fetched,
with t = 0..min(M, 8) equal bytes in front of it (low_blocks).  Every block carries the
sequences it aims for as (position, length); the oracle's stream sizes must be exactly what they give (model_sizes): one token per
sequence in the flags stream, and in the literals stream per sequence its literals, two offset bytes and the length escapes."""
import functools

import producer_chain_inputs as chain_inputs
import producer_tail_inputs as tail_inputs
import util
from producer_tail_inputs import MFLIMIT, _Builder, _le24, visit_pos

LEVELS = (10, 30)
BACK_T = tuple(range(9))             # equal bytes in front of position and candidate (cbk)
BACK_R = (0, 1, 7, 8, 9)             # P - anchor
BACK_PER_BLOCK = 9


def stream_sizes(out):
    """(sequences, literals-stream bytes) of every sub-block of a compressed block; None for one stored raw (see
    producer_tail_inputs.seq_counts for the layout)."""
    i, sizes = 1, []
    while i < len(out):
        res = out[i]
        i += 1
        if res == 128:
            i += 3 + _le24(out, i)
            sizes.append(None)
            continue
        i += 3 + _le24(out, i)
        got = {}
        for bit in (4, 8, 2, 1):
            n = _le24(out, i)
            i += 6 + _le24(out, i + 3) if res & bit else 3 + n
            got[bit] = n
        sizes.append((got[2], got[1]))
    assert i == len(out)
    return sizes


def _ext(present, v):
    return 0 if not present else 1 if v < 254 else 3 if v < 65536 else 4


def model_sizes(seqs, n):
    """What the sequences (position, length) of a one-sub-block input of n bytes put into the flags and literals streams
    (lz_lz4_record_bytes in lz_block.h)."""
    pos = nlit = 0
    for P, ml in seqs:
        L = P - pos
        assert L >= 0 and ml >= 4, (P, ml, pos)
        nlit += _ext(L >= 15, L - 15) + L + 2 + _ext(ml - 4 >= 15, ml - 4 - 15)
        pos = P + ml
    return len(seqs), nlit + n - pos


class _B(_Builder):
    """producer_tail_inputs' builder with words that are defined as literals (every position inserted when they stand less than 62
    bytes behind a match) and come back as one sequence."""

    def define(self, w):
        self.raw(w).noise(1)
        return w

    def again(self, w, back=0):
        self.seqs.append((len(self.b) - back, len(w) + back))
        return self.raw(w)

    def anchor(self, tail=b""):
        """A 40-byte word (+ tail) and the word again: longer than a candidate batch resolves, so it is its round's last winner and the
        next round starts right behind it."""
        w = self.define(self.r.randbytes(40) + tail)
        return self.noise(3).again(w)

    def zeros(self, run_start, v):
        """120 zero bytes inside a run whose first visit is at run_start and whose next visit is number v: found where the second
        visit inside them meets the first one's entry, extended backwards to the step behind their start.  The parse is back at
        step 1 behind them."""
        z = len(self.b)
        while visit_pos(run_start, v) < z:
            v += 1
        step = visit_pos(run_start, v + 1) - visit_pos(run_start, v)
        self.raw(bytes(120))
        self.seqs.append((z + step, 120 - step))
        return self


def _windows(B, count, start=None, words=None):
    """Behind the last match: a run of noise, and from visit 514 on (step 9) `count` windows Y (9 bytes) + X (10 bytes) with X at a
    visited position: the 8 positions in front of X are stepped over.  start: the run's first visit, when literals already stand
    behind the match; words: the (Y, X) to place, else random ones.  Returns the windows and (run start, next visit number)."""
    start = len(B.b) + 1 if start is None else start
    v, out = 514, []
    for k in range(count):
        while visit_pos(start, v) - 9 < len(B.b) + 1:
            v += 1
        p = visit_pos(start, v)
        B.noise(p - 9 - len(B.b))
        Y, X = words[k] if words else (B.r.randbytes(9), B.r.randbytes(10))
        B.raw(Y + X)
        out.append((Y, X))
    B.noise(12)
    return out, start, v


def _back_case(B, Y, X, t, r, chained, behind=None):
    """X again, t equal bytes in front of it, r bytes behind the sequence before it.  chained: that sequence is an 8-byte word three
    literals behind an anchor match, so it is the round's first winner, is pushed inside the chain pass, and X is the second winner of
    the same round: its room is counted from the new anchor.  Otherwise the anchor match itself ends r bytes in front of X.
    behind: a word defined earlier, placed right behind X: an accepting lane at the lane X ends in."""
    eq = Y[9 - t:] if t else b""
    over = eq[:max(0, t - r)]                        # equal bytes that lie inside the sequence before
    if chained:
        w = B.define(B.r.randbytes(8) + over)
        B.anchor().noise(3).again(w)
    else:
        B.noise(8).anchor(over)
    B.raw(eq[len(over):]) if t > r else B.noise(r - t).raw(eq)
    B.again(X, back=min(t, r))
    if behind is not None:
        B.again(behind)
    B.noise(5)


def _exact(data, seqs):
    """The oracle alone gives the sequences the block aims for, at both levels."""
    want = model_sizes(seqs, len(data))
    return all(stream_sizes(util.oracle_compress(data, level)) == [want] for level in LEVELS)


def _search(make, seeds):
    for seed in seeds:
        B = make(seed)
        data = B.noise(30).bytes()
        if _exact(data, B.seqs):
            return data, tuple(B.seqs)
    raise AssertionError("no seed gives the sequences aimed for")


@functools.lru_cache(maxsize=None)
def back_blocks():
    """(name, data, sequences, cases): cbk 0..8 against P - anchor in {0, 1, 7, 8, 9}, as a round's first and as a chained winner.
    (t, r) = (8, 9) is the unresolved case: 8 equal bytes with room beyond them, finished by lz_count_back."""
    cases = [(t, r, c) for c in (False, True) for t in BACK_T for r in BACK_R]
    out = []
    for k in range(0, len(cases), BACK_PER_BLOCK):
        part = cases[k:k + BACK_PER_BLOCK]

        def make(seed):
            B = _B(seed).saver()
            wins, start, v = _windows(B, len(part))
            B.zeros(start, v).noise(20)
            for (Y, X), (t, r, c) in zip(wins, part):
                _back_case(B, Y, X, t, r, c)
            return B
        data, seqs = _search(make, range(7000 + 100 * k, 7000 + 100 * k + 100))
        out.append(("back%02d" % (k // BACK_PER_BLOCK), data, seqs, tuple(part)))
    return tuple(out)


LOW_M = tuple(range(10))             # candidate positions where nothing, or less than 8 bytes, can be fetched in front
LOW_CASES = tuple((M, t) for M in LOW_M for t in BACK_T if t <= M)


@functools.lru_cache(maxsize=None)
def low_blocks():
    """(name, data, sequences, (M, t)): a candidate at position M = 0..9 of the block with t = 0..min(M, 8) equal bytes in front of
    it and of the position it is found from.  X stands at M, all of it literals of the block's first run (every position inserted).
    Later the t bytes in front of M and X come back in a step-9 window with X at the visited position: the match is found at X with
    candidate M and extends backwards over t bytes, down to the block's first byte when t = M.  For 0 < M < 8 the lane fetched
    nothing and reports "open": lz_count_back gives the length; M = 0 has no room; M = 8 with t = 8 is exact for lz_back_from (the
    room ends with the fetched bytes) and open for lz_back_lane; M = 9 with t = 8 is open for both."""
    out = []
    for M, t in LOW_CASES:
        def make(seed):
            B = _B(seed)
            X = B.r.randbytes(10)
            B.noise(M).raw(X).noise(20)
            head = bytes(B.b[:M])
            B.saver()
            Y = bytearray(B.r.randbytes(9 - t) + head[M - t:])
            while M > t and Y[8 - t] == head[M - t - 1]:             # the run of equal bytes ends after t
                Y[8 - t] = B.r.randrange(256)
            _windows(B, 1, words=[(bytes(Y), X)])
            P = bytes(B.b).rindex(X)
            B.seqs.append((P - t, 10 + t))
            return B
        data, seqs = _search(make, range(8000 + 100 * M + 10 * t, 8000 + 100 * M + 10 * t + 200))
        assert data[M:M + 10] == data[seqs[-1][0] + t:seqs[-1][0] + t + 10]
        out.append(("low_M%d_t%d" % (M, t), data, seqs, (M, t)))
    return tuple(out)


def _pair_at(g, la, lb, cut=None, lead=0):
    """Behind an anchor match: g literals, a word of la bytes and one of lb bytes right behind it.  lead: two literals and `lead`
    words of 5 bytes come first (the pair's lanes move up by 1 + 5 * lead: with lead = 2 the first word of the pair is the round's
    third chained sequence if it chains at all).  cut = d: the block ends so that the first word of the pair ends at mflimit + d."""
    def make(seed):
        B = _B(seed).saver().noise(4)
        a, b = B.define(B.r.randbytes(la)), B.define(B.r.randbytes(lb))
        pre = [B.define(B.r.randbytes(5)) for _ in range(lead)]
        B.anchor()
        if lead:
            B.noise(2)
        for w in pre:
            B.again(w)
        B.noise(g).again(a).again(b)
        return B
    for seed in range(9000 + 64 * g + la + lb, 9400 + 64 * g + la + lb):
        B = make(seed)
        if cut is None:
            data, seqs = B.noise(30).bytes(), list(B.seqs)
        else:
            end_a = B.seqs[-2][0] + la
            n = end_a - cut + MFLIMIT
            data, seqs = B.noise(30).bytes()[:n], list(B.seqs[:-1])
        if _exact(data, seqs):
            return data, tuple(seqs)
    raise AssertionError("pair_at")


def _later_round(rounds, pair):
    """Behind an anchor match `rounds` rounds find nothing; a word a (8 bytes) then stands at a visited position P of the next round,
    in lane w.  pair: words b and c right behind it, at P + 8 and P + 16.  The round's step is 2, so b stands in lane w + 4 and c in
    lane w + 8 = w + ml: an accepting lane where a chain pass looks for the next winner, in a later round, which must not chain —
    a pass that chained here would go from a to c and lose b."""
    def make(seed):
        B = _B(seed).saver().noise(4)
        a, b, c = (B.define(B.r.randbytes(8)) for _ in range(3))
        B.anchor()
        start = len(B.b) + 1
        v = 64 * rounds + 4
        step = visit_pos(start, v + 1) - visit_pos(start, v)
        B.noise(visit_pos(start, v) - len(B.b)).again(a)
        if pair:
            assert step == 2
            B.again(b).again(c)
        return B
    return _search(make, range(9500 + 10 * rounds + pair, 9900 + 10 * rounds + pair))


def _unresolved_then_word():
    """The fold of an unresolved backward length into the chain pass's test of the end lane.  First round of a run: X in lane 10 with
    8 equal bytes in front of it and of its candidate and 9 bytes of room (the lane reports "open": unresolved), a forward length the
    batch resolves (10), and a word right behind it, in lane 20 = the lane X ends in: an accepting lane the pass would chain to.  It
    must leave instead, and lz_count_back gives the 8."""
    def make(seed):
        B = _B(seed).saver()
        start = len(B.b) + 1
        b = B.define(B.r.randbytes(8))
        wins, start, v = _windows(B, 1, start=start)
        B.zeros(start, v).noise(20)
        _back_case(B, wins[0][0], wins[0][1], 8, 9, False, behind=b)
        return B
    return _search(make, range(9700, 9900))


def _tail_block(tail):
    """A run that ends at mflimit, `tail` bytes behind the last match: the last round's valid lanes are a proper prefix — of the
    run's first round (tail < 83) or of a later one."""
    for seed in range(9950 + tail, 10150 + tail):
        B = _B(seed).saver().noise(4)
        B.anchor()
        data = B.noise(tail).bytes()
        if _exact(data, B.seqs):
            return data, tuple(B.seqs)
    raise AssertionError("tail_block")


def _ends_in_match(seed=9990):
    """The last sequence ends inside the last MFLIMIT bytes: the loop is left behind a winner (fast.h:143)."""
    def make(s):
        B = _B(s).saver().noise(4)
        a = B.define(B.r.randbytes(12))
        return B.anchor().noise(6).again(a)
    for s in range(seed, seed + 200):
        B = make(s)
        data = B.noise(17).bytes()
        if _exact(data, B.seqs):
            return data, tuple(B.seqs)
    raise AssertionError("ends_in_match")


TAILS = (21, 25, 40, 83, 84, 100, 150, 230)
TINY = (21, 22, 84)


@functools.lru_cache(maxsize=None)
def chain_blocks():
    """(name, data, sequences or None)."""
    out = []
    for l1 in (63, 64, 65):                                             # two 5-byte words in lanes 3-12, winner in lane 13 + g, 8 bytes
        out.append(("l1_%d" % l1,) + _pair_at(l1 - 21, 8, 8, lead=2))
    for d in (0, 1):
        out.append(("ipn_mflimit%+d" % d,) + _pair_at(3, 8, 8, cut=d))
    out.append(("long_first",) + _pair_at(3, 30, 8))
    out.append(("long_second",) + _pair_at(3, 8, 30))
    out.append(("unresolved_then_word",) + _unresolved_then_word())
    out.append(("second_round_pair",) + _later_round(1, True))
    out.append(("winner_nowinner_winner",) + _later_round(1, False))
    out.append(("four_rounds_then_winner",) + _later_round(4, False))
    out.append(("stale_reader", chain_inputs._chain_dense(906, alphabet=b"ab", nwords=24, reps=700), None))
    out += [("tail%d" % t,) + _tail_block(t) for t in TAILS]
    out.append(("ends_in_match",) + _ends_in_match())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_blocks():
    """(name, data).  The 64th push at the tail of a round and inside the chain pass, and the two-sub-block input, are
    producer_tail_inputs' own."""
    out = [(n, d) for n, d, _, _ in back_blocks()] + [(n, d) for n, d, _, _ in low_blocks()] + [(n, d) for n, d, _ in chain_blocks()]
    out += [("tiny%d" % n, _B(n).noise(n).bytes()) for n in TINY]
    keep = ("count64_tail", "count64_match", "dense64_0", "dense64_1", "dense128_0", "two_subblocks9000")
    out += [(n, d) for n, d in tail_inputs.all_blocks() if n in keep]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(level):
    return {name: util.oracle_compress(data, level) for name, data in all_blocks()}
