"""Inputs of tests/test_count_trip_emul.py, tests/test_count_trip_gpu.py and tests/count_trip_asan_main.cpp: small blocks built for the
count trips behind a winner of the level-10 producers' round whose candidate batch left a length unresolved
(lizard_amd/csrc/lz_block.h: the late back trip behind LZ_BACK_LATE).

A serial model of the fast parser (`parse`: one table entry per slot, the visit schedule of fast.h:75-84, the probe of ip behind a
match, put(ip - 2)) gives every sequence of a block with its forward and backward length, the winner's position and candidate, and
whether the batch resolves each length (24 bytes forward, or 16 at the end of a sub-block; 8 bytes backward and the room up to the
anchor, lz_back_lane).  Every input is searched with the model until it holds the case it is built for, and the oracle's stream
sizes must be exactly what the model's sequences give (producer_latch_inputs.model_sizes), so the model is checked by the oracle on
every block it is used on.

How a backward length is made.  A stretch of period 3 (three different bytes) has no match while the run's step is 1, 2 or 3: the
slot of a position holds the last visited position of its residue, 3, 6 and 3 bytes back, and candidates nearer than 8 are refused.
With step 4 (193 visits into a run) the first visit finds the one 12 back, and that match extends backwards down to the start of the
stretch, over every byte the run stepped through, and forwards to the stretch's end.  The literals in front of the stretch set the
backward length, its end the forward length.  A stretch that opens the block gives a backward length cut by the candidate's distance
from the block start (at 60 and 192 bytes; _block_start_cut gives 63, 64 and 65 by overwriting table slots).  A backward length cut
by the anchor: producer_latch_inputs' windows for up to 8 bytes, _anchor_cut9 for 9, _anchor_cut_far for 63, 64, 65 and 130."""
import functools

import producer_latch_inputs as latch
import util
from producer_latch_inputs import _B, model_sizes, stream_sizes

LEVELS = (10, 30)
MFLIMIT, LASTLITERALS, SUBBLOCK = 20, 16, 131072
_K = (889523592379 << 24) & (2 ** 64 - 1)


def _hash(data, p):
    return ((int.from_bytes(data[p:p + 8], "little") * _K) & (2 ** 64 - 1)) >> 52


def _off(v):
    if v == 0:
        return 0
    q, t = (v - 1) >> 6, (v - 1) & 63
    return 1 + (32 * q + t) * (q + 1)


def _step(v):
    return 1 if v == 0 else (63 + v) >> 6


def parse(data):
    """Every sequence of the block as a dict: P, M (winner and candidate as found), fwd, back, room (P - anchor), sub-block number,
    fwd_open / back_open (the candidate batch leaves that length unresolved), and the limits of its sub-block."""
    n, tab, out = len(data), {}, []
    for sub, S in enumerate(range(0, n, SUBBLOCK)):
        E = min(S + SUBBLOCK, n)
        if E - S < MFLIMIT + 1:
            break
        mflimit, matchlimit = E - MFLIMIT, E - LASTLITERALS
        low = S - 65535 if S > 65535 else 0

        def probe(p):
            h = _hash(data, p)
            m = tab.get(h)
            tab[h] = p
            return m if m is not None and 8 <= p - m <= 65535 and m >= low and data[m:m + 4] == data[p:p + 4] else None

        tab[_hash(data, S)] = S
        ip, anchor, special = S + 1, S, False
        while True:
            found, start = None, ip
            if special:
                tab[_hash(data, ip - 2)] = ip - 2
                m = probe(ip)
                if m is not None:
                    found = (ip, m)
                start = ip + 1
            v = 0
            while found is None:
                p = start + _off(v)
                if p + _step(v) > mflimit:
                    break
                m = probe(p)
                if m is not None:
                    found = (p, m)
                v += 1
            if found is None:
                break
            P, M = found
            fwd = 4
            while P + fwd < matchlimit and data[P + fwd] == data[M + fwd]:
                fwd += 1
            back = 0
            while P - back > anchor and M - back > 0 and data[P - back - 1] == data[M - back - 1]:
                back += 1
            seen = 24 if P + 24 <= E else 16
            common = 0
            while common < seen and data[P + common] == data[M + common]:
                common += 1
            fwd_open = not (common < seen or matchlimit - P <= seen)
            if M >= 8:
                c = 0
                while c < 8 and data[P - 1 - c] == data[M - 1 - c]:
                    c += 1
                back_open = c == 8 and P - anchor > 8
            else:
                back_open = M > 0 and P - anchor > 0
            out.append(dict(P=P, M=M, fwd=fwd, back=back, room=P - anchor, sub=sub, fwd_open=fwd_open, back_open=back_open,
                            mflimit=mflimit, matchlimit=matchlimit))
            ip = anchor = P + fwd
            if ip > mflimit:
                break
            special = True
    return out


def marks_of(seqs):
    """What the level-10 producer's marks must count for these sequences (lz_block.h, LZ_CT_MARK 8 and 3 / 9): forward trips, back trips."""
    return {"fwd": sum(s["fwd_open"] for s in seqs), "back": sum(s["back_open"] for s in seqs)}


def model_exact(data):
    """The oracle's stream sizes are those of the model's sequences, at both levels (one-sub-block inputs)."""
    seqs = parse(data)
    want = model_sizes([(s["P"] - s["back"], s["fwd"] + s["back"]) for s in seqs], len(data))
    return all(stream_sizes(util.oracle_compress(data, level)) == [want] for level in LEVELS)


def _find(make, want, seeds, exact=True):
    """The first seed whose block holds a sequence for which want(sequence) is true, with the oracle agreeing with the model."""
    for seed in seeds:
        data = make(seed)
        if data is None:
            continue
        hit = [s for s in parse(data) if want(s)]
        if hit and (not exact or model_exact(data)):
            return data, hit[0]
    raise AssertionError("no seed gives the case")


# ---- forward lengths, backward length resolved (0: the bytes in front differ) ------------------------------------------------
FWD = (23, 24, 27, 28, 515, 516, 517, 1100)


def _fwd_block(L):
    def make(seed):
        B = _B(seed).saver().noise(4)
        w = B.define(B.r.randbytes(L))
        B.raw(bytes(B.r.sample(range(256), 8)) * 15).noise(9)         # (period 8 matches at any step: the run over a long word is back at step 1)
        return B.anchor().noise(5).again(w).noise(30).bytes()
    return _find(make, lambda s: s["fwd"] == L and s["back"] == 0 and not s["back_open"] and s["fwd_open"] == (L >= 24), range(100, 300))


# ---- backward lengths from a period-3 stretch ---------------------------------------------------------------------------------
BACK = (7, 8, 9, 63, 64, 65, 130)
BOTH_FWD, BOTH_BACK = (24, 516, 1100), (9, 64, 130)


def _stretch(B, n):
    pat = bytes(B.r.sample(range(256), 3))
    return (pat * (n // 3 + 2))[:n]


def _periodic(back, fwd, seed, tail=30, head=True):
    """An anchor match, about 386 - back literals (seed % 8 moves them), and a period-3 stretch: the model says where the match is
    found; the stretch is cut so that it runs `fwd` bytes on from there.  tail: the bytes behind it."""
    B = _B(seed)
    if head:
        B.saver().noise(4)
    B.anchor()
    g = 390 - back - seed % 8
    if g < 1:
        return None
    B.noise(g)
    s0 = len(B.b)
    body = _stretch(B, 500 + fwd)
    while B.b[-1] == body[2]:                                      # the byte in front of the stretch does not go on backwards
        B.b[-1] = B.r.randrange(256)
    probe = bytes(B.b) + body + bytes(64)
    first = [s for s in parse(probe) if s["P"] >= s0]
    if not first:
        return None
    e = first[0]["P"] + fwd
    B.raw(body[:e - s0])
    nxt = bytearray(B.r.randbytes(max(tail, 1)))
    while nxt[0] == body[(e - s0) % 3]:
        nxt[0] = B.r.randrange(256)
    return bytes(B.b) + bytes(nxt[:tail])


def _back_block(back, fwd=12):
    want = lambda s: s["back"] == back and s["fwd"] == fwd and s["room"] > back and s["fwd_open"] == (fwd >= 24) and s["back_open"] == (back >= 8)
    return _find(lambda seed: _periodic(back, fwd, seed), want, range(200 + back, 300 + back))


def _to_matchlimit():
    """A stretch that runs to the end of the block: the forward count stops at matchlimit, both lengths unresolved."""
    want = lambda s: s["P"] + s["fwd"] == s["matchlimit"] and s["fwd_open"] and s["back_open"]
    return _find(lambda seed: _periodic(64, 700, seed, tail=0), want, range(300, 340))


def _beyond_mflimit():
    """Both unresolved, and the match ends between mflimit and matchlimit: there is no next run (fast.h:143)."""
    want = lambda s: s["mflimit"] < s["P"] + s["fwd"] < s["matchlimit"] and s["fwd_open"] and s["back_open"]
    return _find(lambda seed: _periodic(9, 40, seed, tail=18), want, range(340, 380))


def _block_start(period):
    """The stretch opens the block: the backward length is cut by the candidate's distance from the block start (M >= i)."""
    def make(seed):
        B = _B(seed)
        pat = bytes(B.r.sample(range(256), period))
        B.raw((pat * 400)[:620]).noise(30)
        return B.saver().noise(30).bytes()
    return _find(make, lambda s: s["back"] == s["M"] and s["back"] > 8 and s["room"] > s["back"], range(400 + period, 440 + period))


def _second_subblock():
    """131 072 + 9 000 bytes: producer_tail_inputs' first sub-block (it ends in a long match cut at its matchlimit), and a "both" case
    in the second."""
    import producer_tail_inputs as tail
    head = dict(tail.all_blocks())["two_subblocks9000"][:SUBBLOCK]
    for seed in range(500, 560):
        part = _periodic(64, 516, seed, tail=30)
        if part is None or len(part) > 9000:
            continue
        B = _B(seed + 1000)
        data = head + part + B.noise(9000 - len(part)).bytes()
        hit = [s for s in parse(data) if s["sub"] == 1 and s["fwd_open"] and s["back_open"] and s["fwd"] >= 516 and s["back"] >= 64]
        if hit:
            return data, hit[0]
    raise AssertionError("second_subblock")


def _sweep_inside():
    """The sweep due at 32 768 falls inside a jointly counted match: 31 KiB of noise, zeros that bring the run back to step 1, and a
    stretch that runs over 32 768."""
    def make(seed):
        B = _B(seed).saver()
        B.noise(32768 - 700 - len(B.b)).raw(bytes(120)).noise(9)
        part = _periodic(64, 1100, seed + 7, head=False)
        return None if part is None else bytes(B.b) + part
    want = lambda s: s["P"] < 32768 < s["P"] + s["fwd"] and s["fwd_open"] and s["back_open"]
    return _find(make, want, range(600, 640))


def _anchor_cut9(fwd):
    """A backward length of 9 cut by the anchor, open for the batch (8 equal bytes fetched, room 9).  A window of Y (10 bytes) and X
    (`fwd` bytes) stands where the run's step is 10, X at a visited position: the 9 positions in front of it are stepped over.  Later an
    anchor match ends 9 bytes in front of X again, with Y's bytes in front of it and, as the anchor word's last byte, inside it: 10
    equal bytes, of which the anchor leaves 9."""
    from producer_tail_inputs import visit_pos
    def make(seed):
        B = _B(seed).saver()
        start, v = len(B.b) + 1, 580                                  # visits 577..640 of a run step by 10
        p = visit_pos(start, v)
        B.noise(p - 10 - len(B.b))
        Y, X = B.r.randbytes(10), B.r.randbytes(fwd)
        B.raw(Y + X).noise(12)
        B.raw(bytes(B.r.sample(range(256), 8)) * 15).noise(9)         # (period 8 matches at any step: back at step 1)
        B.noise(8).anchor(Y[:1])
        return B.raw(Y[1:]).raw(X).noise(30).bytes()
    want = lambda s: (s["back"], s["room"], s["fwd"]) == (9, 9, fwd) and s["back_open"] and s["fwd_open"] == (fwd >= 24) and s["M"] >= 10
    data, s = _find(make, want, range(700 + fwd, 760 + fwd))
    assert data[s["P"] - 10] == data[s["M"] - 10]                     # the anchor cuts it, not the bytes
    return data, s


ANCHOR_FAR = (63, 64, 65, 130)


def _anchor_cut_far(cut, ylen):
    """A backward length of `cut` bytes cut by the anchor (producer_tail_inputs._rare_at_64th's way of making entries disappear).  The
    bytes G T stand three times.  G1 T1 are literals early in the block.  G2 T2 are found as one match from them — nothing inside a match is
    inserted but the position two before its end, T2 (fast.h:146) — and Y2 behind them are literals.  G3 T3 Y3 lie more than 65 535 behind
    the first copy, whose entries are dead by then: the run passes G3 as literals until T3 meets the entry at T2, and that match extends
    backwards over G3 — down to the anchor match that ends `cut` bytes in front of T3 and whose last byte is G's first.  cut = 130: T3
    stands at a position the run visits with step 2."""
    def make(seed):
        B = _B(seed)
        G, T, Y = B.r.randbytes(cut + 1), B.r.randbytes(2), B.r.randbytes(ylen)
        B.noise(40).raw(G + T).noise(30)
        x1 = len(B.b) - 30 - len(G + T)
        B.saver(6000)
        B.noise(65535 - 2600 - len(B.b))
        B.raw(bytes(B.r.sample(range(256), 8)) * 15).noise(20)        # (period 8 matches at any step: back at step 1)
        B.copy(x1, len(G + T)).raw(Y)
        B.avoid = None
        B.noise(9)
        while len(B.b) <= x1 + 65535 + 8 + len(G):
            B.noise(64)
        B.raw(bytes(B.r.sample(range(256), 8)) * 15).noise(9)
        B.noise(8).anchor(G[:1])
        return B.raw(G[1:] + T + Y).noise(30).bytes()
    want = lambda s: (s["back"], s["room"], s["fwd"]) == (cut, cut, 2 + ylen) and s["back_open"] and s["fwd_open"] == (2 + ylen >= 24)
    data, s = _find(make, want, range(800 + cut, 830 + cut))
    assert data[s["P"] - cut - 1] == data[s["M"] - cut - 1]           # the anchor cuts it, not the bytes
    return data, s


@functools.lru_cache(maxsize=None)
def far_cases():
    """(name, data, sequence): the anchor cuts of 63, 64, 65 and 130 bytes, each with the forward length resolved (12) and open (32).
    About 70 KiB each: an entry only dies of age."""
    return tuple(("anchor_cut%d_f%d" % (c, 2 + y),) + _anchor_cut_far(c, y) for c in ANCHOR_FAR for y in (10, 30))


START_M = (63, 64, 65)


def _block_start_cut(M, wlen):
    """A backward length of M bytes cut by the candidate's distance M from the block start.  The block opens with Z (M bytes) and a word W:
    the first run inserts every one of these positions.  The entries of positions 0 .. M - 1 are then overwritten one by one: for each,
    five bytes with the same table slot and other bytes stand as literals right behind an anchor match, where every position is visited
    (the table has one entry per slot).  W's entry, at M, is left alone.  Z W again, one literal behind an anchor match: the run finds
    nothing on its way through Z and meets W with the candidate at M; the match extends backwards over all of Z, to the block's first
    byte.  M = 65: W then stands at the first position the run visits with step 2."""
    def make(seed):
        B = _B(seed)
        Z, W = B.r.randbytes(M), B.r.randbytes(wlen)
        B.raw(Z + W).noise(30).saver()
        head = bytes(B.b[:M + 8])
        killers = []
        for q in range(M):
            h = _hash(head, q)
            while True:
                k = B.r.randbytes(5)
                if k[:4] != head[q:q + 4] and _hash(k + bytes(3), 0) == h:
                    break
            killers.append(k)
        for i in range(0, M, 10):
            B.noise(4).anchor().noise(2)
            for k in killers[i:i + 10]:
                B.raw(k)
        B.noise(8).anchor().noise(1)
        return B.raw(Z + W).noise(30).bytes()
    want = lambda s: s["M"] == M and s["back"] == M and s["room"] > M and s["back_open"] and s["fwd"] == wlen and s["fwd_open"] == (wlen >= 24)
    return _find(make, want, range(900 + M, 960 + M))


@functools.lru_cache(maxsize=None)
def start_cases():
    """(name, data, sequence): candidates 63, 64 and 65 bytes from the block start, each with the forward length resolved and open."""
    return tuple(("start_cut%d_f%d" % (M, w),) + _block_start_cut(M, w) for M in START_M for w in (12, 32))


@functools.lru_cache(maxsize=None)
def cases():
    """(name, data, the sequence the block is built for)."""
    out = [("fwd%d" % L,) + _fwd_block(L) for L in FWD]
    out += [("back%d" % b,) + _back_block(b) for b in BACK]
    out += [("both_f%d_b%d" % (f, b),) + _back_block(b, f) for f in BOTH_FWD for b in BOTH_BACK]
    out.append(("to_matchlimit",) + _to_matchlimit())
    out.append(("beyond_mflimit",) + _beyond_mflimit())
    out += [("block_start_p%d" % d,) + _block_start(d) for d in (3, 7)]
    out.append(("sweep_inside",) + _sweep_inside())
    out += [("anchor_cut9_f%d" % f,) + _anchor_cut9(f) for f in (12, 40)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def anchor_cases():
    """producer_latch_inputs' windows: equal bytes t = 0..8 in front of winner and candidate against a room of r = 0, 1, 7, 8, 9 up to
    the anchor (8 with room 8 resolved by the batch, 8 with room 9 open), and candidates at 0..9 bytes from the block start."""
    return tuple((n, d) for n, d, _, _ in latch.back_blocks()) + tuple((n, d) for n, d, _, _ in latch.low_blocks())


@functools.lru_cache(maxsize=None)
def second_subblock():
    return ("second_subblock",) + _second_subblock()


@functools.lru_cache(maxsize=None)
def all_blocks():
    """(name, data) of everything, the two-sub-block input last."""
    return tuple((n, d) for n, d, _ in cases()) + tuple((n, d) for n, d, _ in far_cases() + start_cases()) + anchor_cases() + (second_subblock()[:2],)


def device_batch(data, bs, level):
    """`data` cut into blocks of bs bytes (the last one shorter) through LizardGPU_compressBlocks_device; the outputs."""
    import numpy as np
    import torch
    from lizard_amd import api
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    dst, sizes, stride = api.compress_blocks_device(src, bs, level)
    torch.cuda.synchronize()
    out, sz = dst.cpu().numpy(), sizes.cpu().numpy()
    return [out[i * stride:i * stride + int(sz[i])].tobytes() for i in range(len(sz))]


@functools.lru_cache(maxsize=None)
def expected(level):
    return {name: util.oracle_compress(data, level) for name, data in all_blocks()}
