"""Inputs of tests/test_producer_tail_emul.py and tests/test_producer_tail_gpu.py: blocks built for what happens BEHIND a winner in
the level-10 producers' round (lizard_amd/csrc/lz_block.h, lz_parse_fast with LANEFORMS): the sequence list's tail kept in a 64-lane
register table (a store every 64 sequences and at the end of the sub-block), the one test for everything rare behind a winner, and
the table sweeps, whose test no longer stands at the head of every round.

How the blocks are made.  noise() bytes are found nowhere else (up to chance).  A `unit` is a literal run followed by a copy of
bytes that lie a few positions back in that same run: every position of a run of fewer than 64 literals behind a match is visited
and inserted, so the copy is found at its first byte — one sequence per unit, of known position and length (the bytes in front of
and behind a copy are chosen so that it extends neither way).  The hash table of these levels has 4 096 slots, so an entry can be
lost to a later position; every builder therefore ASSERTS with the oracle the sequence count it aims for (seq_counts: the length of
the flags stream — one token per sequence) and the seeds below are the first ones for which it holds.  A sub-block is stored
compressed only if it saves 512 bytes + 1/32 of its size, so each opens with a phrase of noise and the phrase again: one long match,
the sub-block's first sequence."""
import functools
import random

import util

LEVELS = (10, 30)                # the producer / consumer kernel; level 30 keeps the LDS ring and the parent's tail
COUNTS = (1, 63, 64, 65, 127, 128, 129)
MFLIMIT = 20                     # LZ_MFLIMIT
SUBBLOCK = 131072
SWEEP_EVERY = 32768


def _le24(b, i):
    return b[i] | b[i + 1] << 8 | b[i + 2] << 16


def seq_counts(out):
    """Sequences of every sub-block of a compressed block: the length of its flags stream (lizard_decompress.c:161-265: level byte,
    then per sub-block a flag byte and the streams len / offset16 / offset24 / flags / literals, each LE24 length + bytes, or LE24
    decoded length + LE24 compressed length + huff0 bytes when its flag bit is set).  None for a sub-block stored raw."""
    i, counts = 1, []
    while i < len(out):
        res = out[i]
        i += 1
        if res == 128:
            i += 3 + _le24(out, i)
            counts.append(None)
            continue
        i += 3 + _le24(out, i)                              # `len`: always raw
        for bit in (4, 8, 2, 1):
            n = _le24(out, i)
            i += 6 + _le24(out, i + 3) if res & bit else 3 + n
            if bit == 2:
                counts.append(n)
    assert i == len(out)
    return counts


class _Builder:
    def __init__(self, seed):
        self.r = random.Random(seed)
        self.b = bytearray()
        self.seqs = []               # (position, length) of every copy that is meant to be one sequence, in order
        self.avoid = None            # the byte that would extend the last copy forwards

    def noise(self, n):
        if n:
            x = bytearray(self.r.randbytes(n))
            while self.avoid is not None and x[0] == self.avoid:
                x[0] = self.r.randrange(256)
            self.b += x
            self.avoid = None
        return self

    def raw(self, data):
        self.b += data
        self.avoid = None
        return self

    def copy(self, src, n):
        """b[src : src + n] again (src + n may reach into the copy itself); the byte in front of it is changed, if need be, so that
        the match does not extend backwards."""
        P = len(self.b)
        while src > 0 and self.b[P - 1] == self.b[src - 1] and not (src <= P - 1 < src + n):
            self.b[P - 1] = self.r.randrange(256)
        for k in range(n):
            self.b.append(self.b[src + k])
        self.seqs.append((P, n))
        self.avoid = self.b[src + n]
        return self

    def saver(self, n=900):
        """n bytes of noise, a few literals, and the n bytes again: one long match (the sub-block is stored compressed)."""
        at = len(self.b)
        self.noise(n).noise(24)
        return self.copy(at, n)

    def unit(self, lit=None, ml=None):
        """12-40 literals and a copy of 8-16 bytes from 8 or more back, inside that literal run."""
        lit = lit or self.r.randrange(12, 41)
        ml = ml or self.r.randrange(8, min(16, lit) + 1)
        d = self.r.randrange(ml, lit + 1)
        self.noise(lit)
        return self.copy(len(self.b) - d, ml)

    def units(self, k):
        for _ in range(k):
            self.unit()
        return self

    def dense(self, k):
        """k copies of 8 bytes, 4-6 literals apart: each repeats the 8 bytes that start at the first literal in front of the copy
        before it (the position the round probes right behind a match — it is inserted), 16-20 back.  Several of them lie in one round."""
        starts = [len(self.b)]                     # the first of the row takes its source from a plain unit's literals
        self.unit(lit=12, ml=8)
        for _ in range(k - 1):
            at = len(self.b)
            self.noise(self.r.randrange(4, 7))
            self.copy(starts[-1], 8)
            starts.append(at)
        return self

    def bytes(self):
        return bytes(self.b)


def _finish(B, end):
    """end = 'tail': 30 literals behind the last sequence (the run behind it is set up and ends at mflimit);
    end = 'match': 17 — the last sequence ends inside the last MFLIMIT bytes, there is no next run (fast.h:143)."""
    return B.noise(30 if end == "tail" else 17).bytes()


def _search(make, want, seeds):
    """The first seed for which the oracle gives the sequence counts `want` (a list, one per sub-block) at both levels."""
    for seed in seeds:
        data = make(seed)
        if all(seq_counts(util.oracle_compress(data, level)) == want for level in LEVELS):
            return data
    raise AssertionError("no seed gives %r sequences" % (want,))


def _count_block(n, end, seed0):
    def make(seed):
        B = _Builder(seed).noise(300 if n == 1 else 0).saver()          # (no block below 2 KiB)
        B.units(n - 1)
        return _finish(B, end)
    return _search(make, [n], range(seed0, seed0 + 400))


def _dense_builder(n, seed):
    """One sequence (the saver), a few units, then copies so close together that rounds chain, n sequences in all."""
    B = _Builder(seed).saver()
    lead = 2 + seed % 5                              # moves the 64th and 128th push through the positions of a chain
    B.units(min(lead, n - 1))
    if n - 1 - lead > 0:
        B.dense(n - 1 - lead)
    return B


def chain_model(seqs, n):
    """Which pushes happen inside the chain loop: a round behind a match that ended at ip holds put(ip - 2) in lane 0, the probe of ip
    in lane 1 and ip + k - 1 in lane k.  A winner in lane w with a length the batch resolves (< 16 here) is pushed inside the loop iff
    its end still has a lane (w + ml <= 63), does not pass mflimit, and the next sequence starts in a lane of the same round.
    Returns (the set of 1-based push numbers made inside the loop, the rounds with three or more such pushes: LZ_STAT mark 8)."""
    inside, rounds3, i = set(), 0, 0
    ip = None
    while i < len(seqs):
        P, ml = seqs[i]
        if ip is None or P - ip + 1 > 63 or ml >= 16:                 # the saver / a later round of the run: no chain
            ip, i = P + ml, i + 1
            continue
        w, nch = max(P - ip + 1, 1), 0
        while i + 1 < len(seqs):
            P, ml = seqs[i]
            P2, ml2 = seqs[i + 1]
            l1 = w + ml
            if ml >= 16 or P + ml > n - MFLIMIT or l1 > 63 or l1 + (P2 - (P + ml)) > 63:
                break
            inside.add(i + 1)
            nch += 1
            rounds3 += nch == 3
            w, i = l1 + (P2 - (P + ml)), i + 1
        P, ml = seqs[i]
        ip, i = P + ml, i + 1
    return inside, rounds3


def _rare_at_64th(ml, back, seed0):
    """63 sequences, then as the 64th — the push that fills the lane table — a match of `ml` bytes (0: a plain 12) whose backward
    extension is `back` bytes (0: none).  back > 0: the bytes X Y stand three times.  X1 Y1 are literals; X2 is found as a match from X1
    (nothing inside a match is inserted, but the position two before its end is, fast.h:146) and Y2 are literals; X3 lies more than
    65 535 behind X1, whose entries are dead by then, and is passed as literals until the entry two before the end of X2 is met: a
    match that extends backwards over X."""
    def make(seed):
        B = _Builder(seed)
        if not back:
            B.saver()
            src = len(B.b)
            B.noise(max(ml, 12) + 9)
            B.units(62)
            B.noise(20).copy(src + 4, ml or 12)
            return _finish(B, "tail")
        X, Y = B.r.randbytes(back + 2), B.r.randbytes(ml or 12)
        B.noise(40).raw(X).noise(30)                                  # X1 (all literals: inserted)
        B.saver(6000)                                                 # sequence 1 (the sub-block must save 512 + 1/32 of its size)
        B.noise(65535 - 2600 - len(B.b))
        B.raw(bytes(120)).noise(20)                                   # sequence 2: a run of zeros brings the parse back to step 1
        B.seqs.append((len(B.b) - 140 + 8, 112))
        x1 = bytes(B.b).index(X)
        B.copy(x1, len(X)).raw(Y)                                     # sequence 3: X2, then Y2 as literals
        B.avoid = None
        B.noise(9).units(60)
        while len(B.b) <= x1 + 65535 + 8:
            B.noise(64)
        B.noise(25)
        B.seqs.append((len(B.b) + len(X) - 2, 2 + len(Y)))
        B.raw(X).raw(Y)                                               # sequence 64
        return _finish(B, "tail")
    return _search(make, [64], range(seed0, seed0 + 400))


def _two_subblocks(extra, seed=77):
    """131 072 + extra bytes.  The first sub-block ends with a partly filled lane table (72 sequences: 8 wait in lanes when it ends)
    and the second starts with an empty one.  Its last sequence is one long match found at position 32 768 exactly, in a round whose
    lane 0 stands below it: the sweep due at 32 768 is made up at 32 769 and the two after it at 65 537 and 98 305, so the next falls
    due at 131 073 — position S + 1 of the second sub-block, where its first round starts.  extra = 13: nothing is parsed there (the
    hand-over alone); extra = 9 000: a second sub-block with sequences of its own."""
    B = _Builder(seed).saver(5000)
    B.units(68)
    B.noise(SWEEP_EVERY - 12 - 42 - 140 - len(B.b)).raw(bytes(120)).noise(20)     # (the zeros bring the parse back to step 1)
    B.seqs.append((len(B.b) - 132, 112))
    B.unit(lit=30, ml=12).noise(12)
    assert len(B.b) == SWEEP_EVERY
    B.copy(SWEEP_EVERY - 12, SUBBLOCK - 16 - SWEEP_EVERY).noise(16)
    assert len(B.b) == SUBBLOCK and len(B.seqs) == 72
    if extra < 100:
        return B.noise(extra).bytes(), [72, None]
    B.saver(3000).units(9)
    return B.noise(extra - (len(B.b) - SUBBLOCK)).bytes(), [72, 10]


def visit_pos(start, v):
    """Position of visit v of a run whose first visit is at `start` (fast.h:75-82)."""
    if v == 0:
        return start
    q, t = (v - 1) >> 6, (v - 1) & 63
    return start + 1 + (32 * q + t) * (q + 1)


def _pair_decides(data, w2, v2, levels=LEVELS):
    """With the oracle alone: the word at w2 (distance 65 535) is found — with its first byte changed the block has one sequence
    less — and the word at v2 (distance 65 536) is not: changing it changes no count."""
    for level in levels:
        base = seq_counts(util.oracle_compress(data, level))
        brk = lambda p: data[:p] + bytes([data[p] ^ 0x55, data[p + 1] ^ 0x55, data[p + 2] ^ 0x55, data[p + 3] ^ 0x55]) + data[p + 4:]
        if None in base or seq_counts(util.oracle_compress(brk(w2), level))[0] != base[0] - 1:
            return False
        if seq_counts(util.oracle_compress(brk(v2), level)) != base:
            return False
    return True


def _sweep_continuation(seed0=5):
    """64 KiB of noise in front of the first match: the sweeps at 32 768 and 65 536 fall due in rounds without a winner.  Words W and V
    stand at two of the first visits of the block's first run; its visits behind 65 536 meet W again at distance 65 535 (found) and,
    behind that match, V at distance 65 536 (dead for the reference)."""
    early = {visit_pos(1, v) for v in range(200)}
    v = 0
    while visit_pos(1, v) < 65537 or not (visit_pos(1, v) - 65535 in early and visit_pos(1, v) - 65535 + 40 in early):
        v += 1
    q = visit_pos(1, v)
    a = q - 65535
    b = a + 40
    for seed in range(seed0, seed0 + 400):
        B = _Builder(seed)
        W, V = B.r.randbytes(16), B.r.randbytes(16)
        B.noise(a).raw(W).noise(b - a - 16).raw(V)
        B.noise(q - len(B.b)).raw(W)
        B.noise(b + 65536 - len(B.b)).raw(V).noise(30)
        data = B.saver(6000).noise(40).bytes()
        if _pair_decides(data, q, b + 65536):
            return data
    raise AssertionError("sweep_continuation")


def _sweep_first_round(delta, seed0):
    """A long match over 32 768 (the sweep is made up at exactly that position, the next is due at 65 536), noise, and a match that
    ends at 65 536 + delta.  V (position 40) comes back at distance 65 536 in the first round behind that match, W (position 64)
    at distance 65 535 in lane 1 of the second: the sweep falls due between the two."""
    for seed in range(seed0, seed0 + 400):
        B = _Builder(seed)
        W, V = B.r.randbytes(16), B.r.randbytes(16)
        B.noise(40).raw(V).noise(8).raw(W).noise(20)
        B.raw(bytes(40000 - len(B.b)))
        B.noise(65536 + delta - 170 - len(B.b))
        B.raw(bytes(120))                                                 # brings the run back to step 1
        B.noise(8).unit(lit=30, ml=12)
        assert len(B.b) == 65536 + delta
        B.noise(40 + 65536 - len(B.b)).raw(V)
        B.noise(64 + 65535 - len(B.b)).raw(W)
        data = B.noise(30).saver(6000).noise(40).bytes()
        if _pair_decides(data, 64 + 65535, 40 + 65536):
            return data
    raise AssertionError("sweep_first_round")


def _sweep_long_match(filler, seed=17):
    """The adversaries of test_gpu_parity.py::test_sweeps_due_inside_long_matches for the 17-bit table, with a shorter head: a long
    match (a run of zeros, a period of 40 000 or of 65 535: one match per sub-block) carries the position over the table's sweep points,
    and what follows probes slots whose entries are 2^17 + 100 positions old with the same bytes and the same check bits."""
    rnd = random.Random(seed)
    x = util.datagen(4000, 0.5, 0.0, 5)
    gap = (1 << 17) + 100 - len(x)
    if filler == "run":
        mid = bytes(gap)
    else:
        pat = rnd.randbytes(filler)
        mid = (pat * (gap // filler + 1))[:gap]
    return x + mid + x + util.datagen(3000, 0.4, 0.0, 6)


# Seeds of the chained inputs, (count, which) -> seed: the first ones from 3000 + 37 * count + 500 * which for which the oracle gives
# the count, chain_model puts push 64 (and push 128, where a 129th sequence follows) inside the chain loop, and — found with the
# emulator, which the model cannot replace here — no chain is stopped by a stale reader: a literal whose table slot holds, by a
# collision among the 4 096 slots, the put of a lane inside the match before it (tests/test_producer_tail_emul.py checks all three).
DENSE_SEEDS = {(63, 0): 5334, (63, 1): 5832, (64, 0): 5373, (64, 1): 5868, (65, 0): 5405, (65, 1): 5906, (127, 0): 7703, (127, 1): 8199,
               (128, 0): 7746, (128, 1): 8243, (129, 0): 7784, (129, 1): 8282}


@functools.lru_cache(maxsize=None)
def dense_cases():
    """(name, data, sequences (position, length), count): the chained inputs with what chain_model needs."""
    out = []
    for (n, k), seed in sorted(DENSE_SEEDS.items()):
        B = _dense_builder(n, seed)
        data = _finish(B, "tail")
        assert all(seq_counts(util.oracle_compress(data, level)) == [n] for level in LEVELS), (n, k)
        out.append(("dense%d_%d" % (n, k), data, tuple(B.seqs), n))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def built():
    """(name, data, sequence counts per sub-block as asserted with the oracle)."""
    out = []
    for n in COUNTS:
        for end in ("tail", "match"):
            out.append(("count%d_%s" % (n, end), _count_block(n, end, 1000 + 10 * n + (end == "match")), [n]))
    out += [(name, data, [n]) for name, data, _, n in dense_cases()]
    for ml, back in ((200, 0), (600, 0), (0, 12), (0, 70), (200, 12), (600, 70)):
        out.append(("rare64_ml%d_back%d" % (ml, back), _rare_at_64th(ml, back, 2000 + ml + back), [64]))
    for extra in (13, 9000):
        data, want = _two_subblocks(extra)
        assert all(seq_counts(util.oracle_compress(data, level)) == want for level in LEVELS), extra
        out.append(("two_subblocks%d" % extra, data, want))
    out.append(("sweep_continuation", _sweep_continuation(), None))
    out += [("sweep_first_round%+d" % d, _sweep_first_round(d, 40 + 10 * d), None) for d in (-1, 0, 1)]
    out += [("sweep_long_%s" % f, _sweep_long_match(f), None) for f in ("run", 40000, 65535)]
    return tuple(out)


def all_blocks():
    return [(name, data) for name, data, _ in built()]


@functools.lru_cache(maxsize=None)
def expected(level):
    """name -> the oracle's output; computed once per level and shared."""
    return {name: util.oracle_compress(data, level) for name, data in all_blocks()}
