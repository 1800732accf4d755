"""CPU: lz_put_stream_huf (lizard_amd/csrc/lz_huf.h) on the SIMT emulator over the named streams of tests/huf_stream_inputs.py, byte
for byte against the oracle's HUF_compress under the accept rule of Lizard_writeStream — and which paths of the stage those streams
reach (the LZ_STAT marks of lz_huf.h).  tests/test_huf_stream_gpu.py runs the same streams through the stage on the device, where
nothing can count marks: that the set is worth running there is established here."""
import ctypes

import pytest

import huf_stream_inputs as H
import util

CANARY = 0xC3
GUARD = 64

_c = ctypes


def _emulator():
    E = util.emulator()
    E.emul_put_stream_huf.argtypes = [_c.c_void_p, _c.c_int, _c.c_void_p, _c.POINTER(_c.c_int), _c.c_uint]
    E.emul_put_streams_huf.argtypes = [_c.c_void_p, _c.POINTER(_c.c_ulonglong), _c.POINTER(_c.c_int), _c.c_int, _c.c_void_p,
                                       _c.POINTER(_c.c_ulonglong), _c.POINTER(_c.c_int), _c.POINTER(_c.c_int), _c.c_uint]
    E.emul_put_streams_huf.restype = None
    return E


def _marks(E, stats):
    E.emul_stats(stats, 1)
    return {i for i in H.MARKS.values() if stats[i]}


def _check_output(name, buf, n, r, h, want):
    """buf: GUARD canary bytes, the n + 3 bytes of the stream's output, GUARD canary bytes."""
    w, wh = want
    assert (r, h) == (len(w), wh), (name, r, h, len(w), wh)
    assert buf[GUARD:GUARD + r] == w, name
    assert buf[:GUARD] == bytes([CANARY]) * GUARD and buf[GUARD + n + 3:] == bytes([CANARY]) * GUARD, name


@pytest.fixture(scope="module")
def run_one_by_one():
    """Every stream through emul_put_stream_huf (a fresh workspace each): name -> marks it reached; outputs are checked on the way."""
    E = _emulator()
    want = H.expected()
    stats = (_c.c_ulonglong * 64)()
    E.emul_stats(stats, 1)
    reached = {}
    for k, (name, data) in enumerate(H.streams()):
        n = len(data)
        out = _c.create_string_buffer(bytes([CANARY]) * (n + 3 + 2 * GUARD), n + 3 + 2 * GUARD)
        src = _c.create_string_buffer(data, n)
        h = _c.c_int(0)
        r = E.emul_put_stream_huf(src, n, _c.byref(out, GUARD), _c.byref(h), k + 1)
        _check_output(name, out.raw, n, r, h.value, want[name])
        assert src.raw == data, name
        reached[name] = _marks(E, stats)
    return reached


def test_every_stream_equals_the_oracle(run_one_by_one):
    """Byte for byte, the `huffed` flag included; no byte outside the n + 3 bytes at the output position changes (those between
    the returned size and n + 3 are unspecified), and none of the stream."""
    assert len(run_one_by_one) == len(H.streams()) >= 300
    total = sum(len(d) for _, d in H.streams())
    assert total <= 16 << 20, total
    huffed = sum(h for _, h in H.expected().values())
    assert 150 < huffed < len(H.streams()) - 30, huffed        # both ends of the stage are well represented


def test_the_set_reaches_exactly_these_marks(run_one_by_one):
    """Every mark of lz_huf.h but one is reached, and every built stream reaches the path it is in the set for (H.REACHES).

    Not reached, and asserted so — a stream that does reach it must be added to H.REACHES and taken off this list:
      hdr_weights_error (53): hdr = 0 because lz_huf_compress_weights returned the reference's error.  Its sources are
        FSE_normalizeCount's tableLog check (FSE_optimalTableLog never chooses less than that minimum), a weight below 1 in
        FSE_normalizeM2, FSE_writeNCount's remaining < 1 / charnum checks and a table spread that does not end at 0: all of
        them guard against an inconsistent normalisation, which lz_fse_normalize does not produce for <= 13 weight counts that sum
        to the number of symbols.  4 000 random count vectors and this set never reached it.

    Reached, although first thought unreachable: hdr_no_nibbles_above_128 (56).  FSE cannot grow the weights of more than 128
    symbols to maxSym / 2 bytes, but it can refuse them: when all symbols below the last one have ONE weight,
    HUF_compressWeights answers 1, HUF_writeCTable wants a nibble header, and there is none above 128 symbols (hdr_eq192)."""
    reached = set().union(*run_one_by_one.values())
    not_reached = {H.MARKS["hdr_weights_error"]}
    assert reached == set(H.MARKS.values()) - not_reached, sorted(reached ^ (set(H.MARKS.values()) - not_reached))
    used = set()
    for name, marks in run_one_by_one.items():
        for prefix, names in H.REACHES:
            if name.startswith(prefix):
                used.add(prefix)
                missing = {m for m in names if H.MARKS[m] not in marks}
                assert not missing, (name, missing)
    assert used == {p for p, _ in H.REACHES}                   # no rule without a stream
    assert run_one_by_one["uniform_20000"] == {H.MARKS["raw_exit"]}            # "not compressible": no tree, no header
    assert all(not run_one_by_one[name] for name, d in H.streams() if len(d) <= H.MIN_HUF)
    assert H.expected()["fate_accepted"][1] == 1 and H.expected()["fate_raw"][1] == 0


def _run_sequence(E, items, want, seed):
    """items: (name, data) through ONE workspace, in order; every output between canaries in one buffer."""
    n = len(items)
    src_at, out_at, cur_s, cur_o = [], [], 0, GUARD
    for _, d in items:
        src_at.append(cur_s); cur_s += len(d)
        out_at.append(cur_o); cur_o += len(d) + 3 + GUARD
    src = b"".join(d for _, d in items)
    sbuf = _c.create_string_buffer(src, len(src))
    out = _c.create_string_buffer(bytes([CANARY]) * cur_o, cur_o)
    sizes, huffed = (_c.c_int * n)(), (_c.c_int * n)()
    E.emul_put_streams_huf(sbuf, (_c.c_ulonglong * n)(*src_at), (_c.c_int * n)(*[len(d) for _, d in items]), n, out,
                           (_c.c_ulonglong * n)(*out_at), sizes, huffed, seed)
    raw = out.raw
    for i, (name, d) in enumerate(items):
        _check_output(name, raw[out_at[i] - GUARD:out_at[i] + len(d) + 3 + GUARD], len(d), sizes[i], huffed[i], want[name])
    assert sbuf.raw == src


def test_streams_in_sequence_through_one_workspace():
    """The product runs a sub-block's flag stream and then its literal stream through one workspace (lz_write_subblock_seq) and the
    next sub-block's after them, while emul_put_stream_huf hands every stream a workspace filled with 0x77: whatever a stream leaves
    behind (the staging ring over the histogram, the leaf-parent table, the weight header's words) must not matter to the next.
    Pairs (neighbours, and each stream behind one from the other half of the set), then the whole set as one sequence."""
    E = _emulator()
    want = H.expected()
    S = list(H.streams())
    half = len(S) // 2
    for i in range(0, len(S) - 1, 2):
        _run_sequence(E, S[i:i + 2], want, i + 1)
    for i in range(half):
        _run_sequence(E, [S[half + i], S[i]], want, i + 7)
    _run_sequence(E, S, want, 3)
    _run_sequence(E, S[::-1], want, 4)
