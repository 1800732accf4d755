"""Inputs of tests/test_producer_chain_emul.py and tests/test_producer_chain_gpu.py: blocks of 4-140 KiB, each built for one path of
the producers' round (lizard_amd/csrc/lz_block.h, lz_parse_fast) — the loop that takes several sequences out of one round and the
slot schedule of the rounds behind a run's first.

How a round lies over the input.  Behind a match that ends at ip, lane 0 is put(ip - 2), lane 1 the probe of ip, lane k >= 2 the
position ip + k - 1: a match g >= 1 literals behind ip wins in lane g + 1 (g = 0: lane 1).  A run that finds nothing goes on:
slots 64.. of the run are visits 62.., the first 64 visits step by 1, the next 64 by 2, then 3, ...  At sub-block entry there are
no post-match slots: lane k is position S + 1 + k.

Every block opens with a phrase repeated six times, so that the container stores it compressed whatever the rest does (a raw block
would hide the parse; the module checks that with the oracle alone, see assert_all_compressed)."""
import functools
import random

import util

LEVELS = (10, 30, 11, 31)
SPLIT_LEVELS = (10, 30)          # producer / consumer kernel (emul_compress_split); 11 / 31 run as one wave per block
GEN_SIZES = (33 * 1024, 131072 + 13)
MFLIMIT = 20                     # LZ_MFLIMIT: no visit at p with p + step > n - 20, no sequence goes on behind n - 20


class _Builder:
    """Pieces of a block.  noise() bytes are found nowhere else (up to chance); again() repeats an earlier word: a match."""

    def __init__(self, seed):
        self.r = random.Random(seed)
        phrase = self.r.randbytes(256)
        self.b = bytearray(phrase * 6 + util.datagen(2600, 0.5, 0.0, seed))      # (no block below 4 KiB)
        self.words = []

    def noise(self, n):
        self.b += self.r.randbytes(n)
        return self

    def word(self, n):
        """n new bytes, remembered: word number len(words) - 1.  A noise byte behind them keeps words apart."""
        return self.define(self.r.randbytes(n))

    def define(self, w):
        self.words.append(w)
        self.b += w + self.r.randbytes(1)
        return len(self.words) - 1

    def again(self, i):
        self.b += self.words[i]
        return self

    def raw(self, data):
        self.b += data
        return self

    def anchor_match(self):
        """A 40-byte match (longer than the batch resolves: the round's last winner, it leaves through the extend step), so that
        the next round starts behind a match at a known position."""
        i = self.word(40)
        self.noise(3)
        return self.again(i)

    def bytes(self):
        return bytes(self.b)


def _chain_dense(seed, alphabet=None, nwords=48, reps=2500):
    """Short matches (4-12 bytes) 0-3 literals apart: three and more sequences out of one round.  With a small alphabet the same
    five bytes come back inside one round, so a reader finds the put of a lane inside a match: the chain must stop there."""
    B = _Builder(seed)
    r = B.r
    mk = (lambda n: bytes(r.choice(alphabet) for _ in range(n))) if alphabet else r.randbytes
    words = [mk(r.randrange(4, 13)) for _ in range(nwords)]
    for w in words:
        B.raw(w + r.randbytes(1))
    for _ in range(reps):
        B.raw(r.choice(words) + mk(r.randrange(0, 4)))
    return B.noise(64).bytes()


def _dead_set_accumulates():
    """Round behind the anchor match: match A (8 bytes, lanes 3..10) holds the five bytes `k` at lanes 5..9; match B follows at once
    and a third match C behind it; the literal stretch between B and C holds `k` again.  The reader of that `k` lies behind the SECOND
    match and its slot holds the put of a lane inside the FIRST: the dead set of the first pass must still count in the second.
    Second part: the only stale lane is l1 - 2 itself — `k2` sits at the last two bytes of a match and the next three, and again
    right behind; put(ip-2) did happen, so this chain goes on."""
    B = _Builder(901)
    for rep in range(6):
        k = B.r.randbytes(5)
        a = B.define(B.r.randbytes(2) + k + B.r.randbytes(1))
        b, c = B.word(6 + rep), B.word(8)
        B.anchor_match().noise(2).again(a).again(b).noise(1 + rep % 3).raw(k).noise(2 + rep).again(c).noise(9)
    for rep in range(6):
        k2 = B.r.randbytes(5)
        a = B.define(B.r.randbytes(6) + k2[:2])
        c = B.word(8)
        B.anchor_match().noise(1 + rep).again(a).raw(k2[2:]).noise(3).raw(k2).noise(2).again(c).noise(7)
    return B.noise(64).bytes()


def _lane_limits():
    """w + ml = 62, 63 and 64 (a match of 8 bytes g = 53, 54, 55 literals behind the anchor match, a second one right behind it: the
    chained winner sits in lane 62 / 63, or the chain leaves because lane 64 does not exist); a first winner in lane 63 (g = 62);
    a winner in lane 0 of a run's second round (g = 63: visit 62) and in its lane 63."""
    B = _Builder(902)
    for g in (53, 54, 55, 62, 63, 63 + 63, 52, 56):
        for ml in (8, 5, 12):
            a, b = B.word(ml), B.word(7)
            B.anchor_match().noise(g + 8 - ml).again(a).again(b).noise(5)
    return B.noise(64).bytes()


def _backward_to_anchor():
    """A chained winner whose backward extension reaches the new anchor.  The byte in front of the word is a position the first
    occurrence's run stepped over (step 2 stretch, both parities offered), so the hash table never saw it: the second occurrence is
    found at the word and extended backwards over that byte, up to the end of the sequence before it."""
    B = _Builder(903)
    ids = []
    B.anchor_match().noise(80)
    for i in range(8):
        y = B.r.randbytes(1 + i % 2)
        w = B.r.randbytes(9)
        ids.append(B.define(y + w))
        B.noise(1 + i % 2)
    B.noise(40)
    for i in ids:
        a = B.word(6)
        B.anchor_match().noise(4).again(a).again(i).noise(6)
    return B.noise(64).bytes()


def _ends_at_mflimit(delta):
    """The last round's first sequence ends at mflimit + delta and the bytes behind it would match again."""
    B = _Builder(910 + delta)
    a, b = B.word(8), B.word(24)
    B.anchor_match().noise(3).again(a).again(b)
    data = B.bytes()
    cut = len(data) - 24 + MFLIMIT - delta            # position of `b` = n - MFLIMIT + delta
    return data[:cut]


def _run(gap, at_entry):
    """Incompressible stretches of `gap` bytes between matches: runs of two, three, four and about eight rounds.  at_entry: the stretch
    opens the second sub-block (special = 0) instead of following a match (special = 1: lanes 0-2 of a later round straddle two
    values of q)."""
    B = _Builder(920 + gap + at_entry)
    if at_entry:
        B.raw(util.datagen(131072 - len(B.b) - 50, 0.5, 0.0, gap))
        w = B.word(30)
        B.noise(50 - 31)
        assert len(B.b) == 131072
        B.noise(gap).again(w).noise(5)
    for k in range(6):
        w = B.word(20)
        B.anchor_match().noise(gap + k).again(w).noise(3)
    return B.noise(64).bytes()


def _tail(tail):
    """A run that ends at mflimit: `tail` incompressible bytes behind the last match.  The sweep over `tail` puts pv + step on
    mflimit - 1, mflimit and mflimit + 1 at every step width, and the last valid slot into a later round of the run."""
    B = _Builder(940)
    return B.anchor_match().noise(tail).bytes()


def visit_off(v):
    """Offset of visit v from the run's first position and its step (lz_visit_off / lz_visit_step, fast.h:75-82)."""
    if v == 0:
        return 0, 1
    q, t = (v - 1) >> 6, (v - 1) & 63
    return 1 + (32 * q + t) * (q + 1), (63 + v) >> 6


_BOUNDARY_SEED = 961                     # (960: a table collision at level 10 loses the word before visit 300; assert_boundary_decides)
BOUNDARY_VISITS = (100, 150, 300)        # later rounds of the run: step 2, 3 and 5


def _boundary(v, d):
    """A word that is in the table comes back exactly at visit v of the run behind a match, and the block ends so that this visit's
    p + step is mflimit + d.  d = 0: the last valid slot, the word must be found (a match of 4 + step bytes up to the end);
    d = 1: the first slot that is not visited any more, the bytes stay literals.  The slot schedule decides between the two outputs.
    (Only behind a match: a run that opens a sub-block and ends at its mflimit is the whole sub-block, and a sub-block without a
    gain is stored raw whatever the parse was — that end of the schedule cannot be seen in the output.)"""
    B = _Builder(_BOUNDARY_SEED + v)             # (one seed for d = 0 and 1: the same bytes, one position apart in length)
    B.anchor_match().noise(3)            # the word lies in the step-1 stretch behind a match: every position of it is inserted
    w = B.word(32)
    B.noise(40).anchor_match()
    ip = len(B.b)
    off, step = visit_off(v)
    B.noise(1 + off).again(w)            # visit v of the run behind a match is at ip + 1 + f(v)
    p = ip + 1 + off
    return B.bytes()[:p + step - d + MFLIMIT]


TAILS = tuple(t0 + i for t0 in (21, 60, 84, 150, 200, 330, 700) for i in range(4))      # four in a row: both parities of a step-2 stretch, +-1


@functools.lru_cache(maxsize=None)
def generated(size):
    """datagen P50, seeds 8-15."""
    return tuple(util.datagen(size, 0.5, 0.0, seed) for seed in range(8, 16))


@functools.lru_cache(maxsize=None)
def built():
    """(name, data): every one must be stored compressed."""
    out = [("chain_dense", _chain_dense(900)),
           ("chain_dense_ab", _chain_dense(904, alphabet=b"ab", nwords=24)),
           ("chain_dense_abcd", _chain_dense(905, alphabet=b"abcd")),
           ("dead_set_accumulates", _dead_set_accumulates()),
           ("lane_limits", _lane_limits()),
           ("backward_to_anchor", _backward_to_anchor())]
    out += [("ends_at_mflimit%+d" % d, _ends_at_mflimit(d)) for d in (-1, 0, 1)]
    out += [("run%d_%s" % (gap, "entry" if e else "match"), _run(gap, e)) for gap in (70, 130, 200, 700) for e in (0, 1)]
    out += [("tail%d" % t, _tail(t)) for t in TAILS]
    out += [("boundary_v%d%+d" % (v, d), _boundary(v, d)) for v in BOUNDARY_VISITS for d in (0, 1)]
    return tuple(out)


def all_blocks():
    return [("gen%d_s%d" % (size, 8 + i), d) for size in GEN_SIZES for i, d in enumerate(generated(size))] + list(built())


@functools.lru_cache(maxsize=None)
def expected(level):
    """name -> the oracle's output; computed once per level and shared."""
    return {name: util.oracle_compress(data, level) for name, data in all_blocks()}


def assert_boundary_decides():
    """With the oracle alone: the word at the last valid slot is found (the block loses the 4 + step bytes of a match's literals and
    gains a sequence), one position later it is not — told by what the same block costs with the word's first byte changed."""
    for level in LEVELS:
        for v in BOUNDARY_VISITS:
            step = visit_off(v)[1]
            for d in (0, 1):
                data = _boundary(v, d)
                p = len(data) - MFLIMIT + d - step
                other = data[:p] + bytes([data[p] ^ 0x55]) + data[p + 1:]
                a, b = util.oracle_compress(data, level), util.oracle_compress(other, level)
                differs = len(a) != len(b) or sum(x != y for x, y in zip(a, b)) > 1      # more than the changed literal itself
                assert differs == (d == 0), (level, v, d, len(a), len(b))


def assert_all_compressed():
    """With the oracle alone: no input ends as a raw block (level byte + a 4-byte header per stored sub-block), at any level."""
    for level in LEVELS:
        want = expected(level)
        for name, data in all_blocks():
            assert 4096 <= len(data) <= 140 * 1024, (name, len(data))
            assert len(want[name]) < len(data), (level, name, len(want[name]), len(data))

