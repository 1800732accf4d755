"""Differential tests of the block DEcoder (lizard_amd/csrc/lz_unpack.h) on hostile and unusual input.

The oracle is the product's own host decoder (Lizard_decompress_safe, lizard_amd/csrc/lizard_decode_host.c): for every block,
valid or damaged, the wave decoder must return the same size or the same refusal, and the same bytes.  Where the reference
decoder (oracle/_ref) accepts too, its output must agree.  Every decode goes through `guarded_decode`: blocks sit in odd slots
between 0-byte sentinel blocks, the destination is pre-filled with a canary, a guard follows the last slot, and the batch runs
twice with different bytes around every block (a read outside a block would change a result).

CPU: the decoder body on the SIMT emulator (tests/emul) — the twin of every GPU test.  GPU (-m gpu): the gfx950 code object
through LizardGPU_decompressBlocks_device (one launch per capacity), _host (packed) and LizardGPU_decompress_safe.

Hand-built blocks (matches at every offset 1..520, offset edges, huff0 streams of the reference encoder, edited weight headers,
24-bit offsets up to 16 MiB) are checked against `model_decode`, a byte-at-a-time literal / match copy loop.

LIZARD_SOAK_SEED picks the fuzz seed (printed in every failure message)."""
import ctypes
import functools
import os
import random
import struct

import numpy as np
import pytest

import util

C = ctypes
SEED = int(os.environ.get("LIZARD_SOAK_SEED", "20261016"))
ERR = 0xFFFFFFFF
CANARY = 0xC3
GUARD = 4096          # bytes behind the last destination slot
SRC_PAD = 64          # bytes behind every block inside its source slot
REF_LEVELS = list(range(10, 50))
GPU_LEVELS = [10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 30, 31, 32, 33, 34, 35, 36, 37, 38, 40, 41, 42]


# ---------------------------------------------------------------- decoders on the host ----------------------------------------

@functools.lru_cache(maxsize=None)
def product_lib():
    from lizard_amd import _lib
    _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    L.Lizard_decompress_safe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.Lizard_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.Lizard_compress.restype = C.c_int
    L.LizardGPU_decompressBlocks_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.LizardGPU_decompressBlocks_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.LizardGPU_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.LizardGPU_lastError.restype = C.c_char_p
    return L


def need_reference():
    ref = util.reference()
    if ref is None:
        util.need_ref("oracle/_ref/liblizard_ref_reset.so")
    return ref


def host_decode(comp, cap):
    """The product's host decoder with 64 canary bytes on both sides of source and destination: (size or ERR, bytes)."""
    L = product_lib()
    g = 64
    src = (C.c_ubyte * (len(comp) + 2 * g))()
    C.memset(src, 0x5A, len(src))
    C.memmove(C.addressof(src) + g, comp, len(comp))
    out = (C.c_ubyte * (cap + 2 * g))()
    C.memset(out, CANARY, len(out))
    r = L.Lizard_decompress_safe(C.addressof(src) + g, C.addressof(out) + g, len(comp), cap)
    raw = bytes(out)
    assert raw[:g] == bytes([CANARY]) * g and raw[g + cap:] == bytes([CANARY]) * g, "host decoder wrote outside its buffer"
    if r < 0:
        return ERR, b""
    assert r <= cap
    return r, raw[g:g + r]


def ref_decode(comp, cap):
    """The reference decoder; its wild copies get 64 bytes of slack in the buffer, not in the capacity."""
    ref = util.reference()
    out = C.create_string_buffer(cap + 64)
    r = ref.Lizard_decompress_safe(comp, out, len(comp), cap)
    return (ERR, b"") if r < 0 else (r, out.raw[:r])


# ---------------------------------------------------------------- the guarded batch decode ------------------------------------

def _emul_run(src, stride, sizes, dst, cap, seed):
    emu = util.emulator()
    emu.emul_decompress_block.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint]
    out = np.empty(len(sizes), dtype=np.uint32)
    for i, n in enumerate(sizes):
        r = emu.emul_decompress_block(src.ctypes.data + i * stride, int(n), dst.ctypes.data + i * cap, cap, seed + i)
        out[i] = ERR if r < 0 else r
    return out


def _device_run(src, stride, sizes, dst, cap, seed):
    import torch
    L = product_lib()
    s = torch.from_numpy(src).cuda()
    sz = torch.from_numpy(sizes.view(np.int32)).cuda()
    d = torch.from_numpy(dst).cuda()
    o = torch.full((len(sizes),), 0x7A7A7A7A, dtype=torch.int32, device="cuda")
    rc = L.LizardGPU_decompressBlocks_device(s.data_ptr(), stride, sz.data_ptr(), len(sizes), d.data_ptr(), cap, o.data_ptr(), None)
    assert rc == 0, L.LizardGPU_lastError()
    torch.cuda.synchronize()
    dst[:] = d.cpu().numpy()
    return o.cpu().numpy().view(np.uint32).copy()


def _guarded_class(blocks, cap, run, fill, seed):
    k = len(blocks)
    nslots = 2 * k + 1
    stride = (max(len(b) for b in blocks) + SRC_PAD + 7) & ~7
    if fill == "zero":
        src = np.zeros(nslots * stride, dtype=np.uint8)
    else:
        src = np.random.default_rng(seed).integers(0, 256, nslots * stride, dtype=np.uint8)
        src[::7] = 0xFF
    sizes = np.zeros(nslots, dtype=np.uint32)
    for i, b in enumerate(blocks):
        at = (2 * i + 1) * stride
        src[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
        sizes[2 * i + 1] = len(b)
    dst = np.full(nslots * cap + GUARD, CANARY, dtype=np.uint8)
    out = run(src, stride, sizes, dst, cap, seed)
    ctx = "cap %d, seed %d" % (cap, SEED)
    assert (out[0::2] == 0).all(), "a sentinel block decoded to something (%s)" % ctx
    view = dst[:nslots * cap].reshape(nslots, cap)
    touched = np.flatnonzero((view[0::2] != CANARY).any(axis=1))
    assert touched.size == 0, "sentinel slot %d written (%s)" % (2 * touched[0], ctx)
    assert (dst[nslots * cap:] == CANARY).all(), "guard behind the last slot written (%s)" % ctx
    res = []
    for i in range(k):
        r = int(out[2 * i + 1])
        assert r == ERR or r <= cap, "block %d: size %d past its capacity (%s)" % (i, r, ctx)
        row = view[2 * i + 1]
        if r != ERR:
            assert (row[r:] == CANARY).all(), "block %d: accepted with %d bytes, wrote past them (%s)" % (i, r, ctx)
        res.append((r, row.tobytes()))
    return res


def guarded_decode(items, run, seed=SEED):
    """Decode (block, cap) pairs with a slot-form batch runner, one launch per capacity, under every guard check, twice (zeros
    and random bytes around every block).  Returns [(size or ERR, decoded bytes)] in the order of `items`."""
    by_cap = {}
    for idx, (b, cap) in enumerate(items):
        by_cap.setdefault(cap, []).append(idx)
    results = [None] * len(items)
    for cap, idxs in sorted(by_cap.items()):
        blocks = [items[i][0] for i in idxs]
        a = _guarded_class(blocks, cap, run, "zero", seed + cap)
        b = _guarded_class(blocks, cap, run, "random", seed + cap + 1)
        for j, i in enumerate(idxs):
            assert a[j][0] == b[j][0], "item %d: size %d with zeros around the block, %d with random bytes (seed %d)" % (i, a[j][0], b[j][0], SEED)
            if a[j][0] != ERR:
                assert a[j][1] == b[j][1], "item %d: output depends on the bytes around the block (seed %d)" % (i, SEED)
            results[i] = (a[j][0], a[j][1][:a[j][0]] if a[j][0] != ERR else b"")
    return results


def host_form_decode(items):
    """The same pairs through LizardGPU_decompressBlocks_host, packed back to back, one call per capacity."""
    L = product_lib()
    by_cap = {}
    for idx, (b, cap) in enumerate(items):
        by_cap.setdefault(cap, []).append(idx)
    results = [None] * len(items)
    for cap, idxs in sorted(by_cap.items()):
        blocks = [items[i][0] for i in idxs]
        packed = np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint64)
        out = np.full(len(blocks) * cap, CANARY, dtype=np.uint8)
        sz = np.zeros(len(blocks), dtype=np.uint32)
        rc = L.LizardGPU_decompressBlocks_host(packed.ctypes.data, offs.ctypes.data, len(blocks), out.ctypes.data, cap, sz.ctypes.data)
        assert rc == 0, L.LizardGPU_lastError()
        for j, i in enumerate(idxs):
            r = int(sz[j])
            results[i] = (r, out[j * cap:j * cap + r].tobytes() if r != ERR else b"")
    return results


# ---------------------------------------------------------------- the container, walked -------------------------------------

def _le24(v):
    return bytes([v & 255, (v >> 8) & 255, (v >> 16) & 255])


def _rd24(b, p):
    return b[p] | (b[p + 1] << 8) | (b[p + 2] << 16)


def walk(block):
    """Fields of a block (lz_unpack.h:367-398): sub-block flags, every 24-bit length, and per huff0 stream its header byte, jump
    table and the last byte of each of its four bitstreams.  Stops where the block stops making sense."""
    f = {"flag": [], "len": [], "huf_n": [], "huf_c": [], "hdr": [], "jump": [], "end": []}
    n = len(block)
    pos = 1
    while pos < n:
        flag = block[pos]
        f["flag"].append(pos)
        pos += 1
        if pos + 3 > n:
            break
        f["len"].append(pos)
        if flag == 128:
            pos += 3 + _rd24(block, pos)
            continue
        pos += 3 + _rd24(block, pos)                        # the unused len stream
        for bit in (4, 8, 2, 1):                            # off16, off24, flags, literals
            if pos + 3 > n:
                return f
            if not flag & bit:
                f["len"].append(pos)
                pos += 3 + _rd24(block, pos)
                continue
            if pos + 6 > n:
                return f
            sn, c = _rd24(block, pos), _rd24(block, pos + 3)
            f["huf_n"].append(pos)
            f["huf_c"].append(pos + 3)
            p = pos + 6
            if 1 < c < sn and p + c <= n:
                i0 = block[p]
                h = 1 + ((i0 - 127 + 1) // 2 if i0 >= 128 else i0)
                f["hdr"].append(p)
                jt = p + h
                if jt + 6 <= p + c:
                    f["jump"].append(jt)
                    l1, l2, l3 = (struct.unpack_from("<H", block, jt + 2 * k)[0] for k in range(3))
                    ends = [jt + 6 + l1, jt + 6 + l1 + l2, jt + 6 + l1 + l2 + l3, p + c]
                    f["end"] += [e - 1 for e in ends if jt + 6 < e <= p + c]
            pos += 6 + c
    return f


def damage_unstructured(rnd, comp):
    b = bytearray(comp)
    kind = rnd.randrange(5)
    if kind == 0:
        for _ in range(rnd.randrange(1, 4)):
            b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
    elif kind == 1:
        del b[rnd.randrange(1, len(b)) if len(b) > 1 else 0:]
    elif kind == 2:
        k = rnd.randrange(1, 9)
        at = rnd.randrange(len(b))
        b[at:at + k] = rnd.randbytes(k)
    elif kind == 3:
        b += rnd.randbytes(rnd.randrange(1, 21))
    else:
        b[rnd.randrange(min(40, len(b)))] = rnd.randrange(256)
    return bytes(b)


def damage_structured(rnd, comp, fields=None):
    """Hit one field of the container on purpose.  None when the block has no field of the kind drawn."""
    f = fields or walk(comp)
    b = bytearray(comp)
    kind = rnd.choice(["flag", "len", "huf_n", "huf_c", "hdr", "jump", "end"])
    if not f[kind]:
        kind = rnd.choice(["flag", "len"])
        if not f[kind]:
            return None
    p = rnd.choice(f[kind])
    if kind == "flag":
        b[p] = rnd.choice([b[p] ^ 1, b[p] ^ 2, b[p] ^ 4, b[p] ^ 8, b[p] | 16, 128, 0, 15, rnd.randrange(256)])
    elif kind in ("len", "huf_n", "huf_c"):
        v = _rd24(b, p)
        choices = [0, v + 1, max(v - 1, 0), len(b) + rnd.randrange(1, 1000), 0xFFFFFF, rnd.randrange(1 << 24)]
        if kind == "huf_c":
            choices += [_rd24(b, p - 3), 1, 1]               # the stored form, the one-symbol form
        if kind == "huf_n":
            choices += [v + 1, max(v - 1, 0), 131072 + 33]
        b[p:p + 3] = _le24(rnd.choice(choices) & 0xFFFFFF)
    elif kind == "hdr":
        b[p] = rnd.choice([b[p] ^ 1, (b[p] + 1) & 255, (b[p] - 1) & 255, 127, 128, 129, 255, 0, 1, 4, rnd.randrange(256)])
    elif kind == "jump":
        k = rnd.randrange(6)
        b[p + k] = rnd.choice([(b[p + k] + 1) & 255, (b[p + k] - 1) & 255, 0, 255, rnd.randrange(256)])
    else:
        b[p] = rnd.choice([0, b[p] ^ (1 << rnd.randrange(8)), 0x80, 1, b[p] >> 1])
    return bytes(b)


# ---------------------------------------------------------------- sources and fuzz cases ------------------------------------

def _sample(rnd, n):
    kind = rnd.randrange(4)
    if kind == 0:
        return util.datagen(n, rnd.choice([0.2, 0.5, 0.8]), 0.0, rnd.randrange(1 << 30))
    if kind == 1:
        return bytes(rnd.choice(b"abcd") for _ in range(n))
    if kind == 2:
        return ((b"the quick brown fox jumps over the lazy dog %d. " % rnd.randrange(100)) * (n // 40 + 1))[:n]
    return util.datagen(n, 0.9, 0.3, rnd.randrange(1 << 30))


def _ref_compress(data, level):
    out, r = util.compress_with(util.reference().Lizard_compress, data, level)
    assert r > 0, (level, len(data))
    return out


def fuzz_cases(seed, sizes, per_base, levels_ref, levels_product, product_compress, shared_cap=1100):
    """(block, cap, plain or None, label) items: for every size, one sample compressed at every level, then damaged blocks per
    capacity class n, n+100, n-1, n-100, n-5000, with the intact block interleaved in every class.  Sizes up to shared_cap - 100
    take shared_cap in place of n+100: one launch then holds more slots than the device has waves, and waves claim block after
    block (lz_claim_index), refused ones included."""
    rnd = random.Random(seed)
    items = []
    for n in sizes:
        data = _sample(rnd, n)
        bases = [(_ref_compress(data, lv), "ref L%d" % lv) for lv in levels_ref]
        bases += [(product_compress(data, lv), "product L%d" % lv) for lv in levels_product]
        caps = [c for c in dict.fromkeys([n, n + 100 if n + 100 > shared_cap else shared_cap, n - 1, n - 100, n - 5000]) if c > 0]
        for comp, label in bases:
            fields = walk(comp)
            for cap in caps:
                items.append((comp, cap, data, label + " intact"))
                for j in range(per_base):
                    bad = damage_structured(rnd, comp, fields) if j % 2 else None
                    bad = bad if bad is not None else damage_unstructured(rnd, comp)
                    items.append((bad, cap, None, label + " damaged"))
    return items


def emul_decode(comp, cap):
    return guarded_decode([(comp, cap)], _emul_run)[0]


def check_differential(items, results, twin=None):
    """Every result equal to the host decoder's; intact blocks that fit decode to their input; where the reference accepts as
    well, the same bytes.  One difference is by design: the host decoder keeps the reference's wild-copy margins (16 bytes of
    room behind a sequence in the output and behind a literal run in its stream), the wave decoder does not
    (test_decompress._short_tail_vectors).  A block only the wave decoder accepts must then decode on `twin` (the emulated wave
    decoder, for the device) to the same result.  Returns the counts."""
    have_ref = util.reference() is not None
    cnt = {"damaged": 0, "accepted": 0, "refused": 0, "equal_to_host": 0, "wave_only_accepts": 0, "ref_both_accept": 0,
           "ref_only_accepts": 0, "intact": 0}
    for i, ((block, cap, plain, label), (r, out)) in enumerate(zip(items, results)):
        hr, hout = host_decode(block, cap)
        ctx = "item %d (%s, %d bytes, cap %d, seed %d)" % (i, label, len(block), cap, SEED)
        if hr == ERR and r != ERR:
            cnt["wave_only_accepts"] += 1
            if twin is not None:
                assert twin(block, cap) == (r, out), "%s: accepted by the device only, the emulated wave decodes differently" % ctx
        else:
            assert r == hr, "%s: wave decoder %s, host decoder %s" % (ctx, "refused" if r == ERR else r, "refused" if hr == ERR else hr)
            assert out == hout, "%s: wave decoder and host decoder disagree on the bytes" % ctx
            cnt["equal_to_host"] += 1
        if plain is not None:
            cnt["intact"] += 1
            if cap >= len(plain):
                assert r == len(plain) and out == plain, "%s: valid block not decoded exactly" % ctx
            else:
                assert r == ERR, "%s: valid block accepted into a slot too small" % ctx
        else:
            cnt["damaged"] += 1
            cnt["accepted" if r != ERR else "refused"] += 1
        if have_ref:
            rr, rout = ref_decode(block, cap)
            if rr != ERR and r != ERR:
                cnt["ref_both_accept"] += 1
                assert rr == r and rout == out, "%s: accepted by both, the reference decodes differently" % ctx
            elif rr != ERR:
                cnt["ref_only_accepts"] += 1
    return cnt


# ---------------------------------------------------------------- hand-built blocks and the model ------------------------------

def _esc(v):
    if v < 254:
        return bytes([v])
    if v < 65536:
        return bytes([254]) + struct.pack("<H", v)
    return bytes([255]) + _le24(v)


def _container(level, flags, lits, off16=b"", off24=b"", lits_huf=None):
    """One sub-block, streams raw; lits_huf = (n, payload) stores the literals stream as huff0 (flag bit 1)."""
    head = bytes([level, 1 if lits_huf else 0]) + _le24(0) + _le24(len(off16)) + off16 + _le24(len(off24)) + off24 + _le24(len(flags)) + flags
    if lits_huf:
        return head + _le24(lits_huf[0]) + _le24(len(lits_huf[1])) + lits_huf[1]
    return head + _le24(len(lits)) + lits


def encode(seqs, last, lz4):
    """Sequences (literals, match length, offset, form) -> block.  form: 'lz4' (token + inline offset), 'new16' / 'rep' (LIZv1
    token >= 32 with a new 16-bit or the repeat offset), 'off24' (LIZv1 token < 32, match length >= 16, literals in front of it go
    in a literal-only repeat token)."""
    flags, lits, o16, o24 = bytearray(), bytearray(), bytearray(), bytearray()
    for L, ml, off, form in seqs:
        if form == "lz4":
            flags.append(min(len(L), 15) | (min(ml - 4, 15) << 4))
            lits += (_esc(len(L) - 15) if len(L) >= 15 else b"") + L + struct.pack("<H", off)
            lits += _esc(ml - 19) if ml - 4 >= 15 else b""
        elif form in ("new16", "rep"):
            tok = (0x80 if form == "rep" else 0) | (min(ml, 15) << 3) | min(len(L), 7)
            assert tok >= 32
            flags.append(tok)
            lits += (_esc(len(L) - 7) if len(L) >= 7 else b"") + L + (_esc(ml - 15) if ml >= 15 else b"")
            if form == "new16":
                o16 += struct.pack("<H", off)
        else:
            if L:
                flags.append(0x80 | min(len(L), 7))
                lits += (_esc(len(L) - 7) if len(L) >= 7 else b"") + L
            assert ml >= 16
            if ml - 16 < 31:
                flags.append(ml - 16)
            else:
                flags.append(31)
                lits += _esc(ml - 47)
            o24 += _le24(off)
    lits += last
    return _container(10 if lz4 else 20, bytes(flags), bytes(lits), bytes(o16), bytes(o24))


def model_decode(seqs, last, prefix=b""):
    """The plain model: literals appended, then every match byte copied one at a time from `off` bytes back.  None if a match
    reaches before the output (or has offset 0)."""
    out = bytearray(prefix)
    for L, ml, off, _ in seqs:
        out += L
        if off == 0 or off > len(out):
            return None
        for _ in range(ml):
            out.append(out[-off])
    return bytes(out + last)


LENS = list(range(4, 81)) + list(range(255, 261))


def _match_seqs(rnd, offsets, form):
    """Every offset with lengths from 4..80 / 255..260 (all of them for offsets below 9), 1000 and 70000 now and then, each match
    starting at an output position chosen modulo 64 (so every residue modulo 8 comes round)."""
    seqs = [(rnd.randbytes(600), 4 if form != "off24" else 16, 600, form if form != "rep" else "new16")]
    pos = 604 if form != "off24" else 616
    j = 0
    for off in offsets:
        lens = LENS + [1000, 70000] if off < 9 else [LENS[(off * 7) % len(LENS)], LENS[(off * 13 + 5) % len(LENS)], 255 + off % 6]
        if off >= 9 and off % 8 == 0:
            lens.append(1000)
        if off >= 9 and off % 64 == 0:
            lens.append(70000)
        for ml in lens:
            j += 1
            target = (off * 11 + j * 17) % 64
            L = rnd.randbytes((target - pos) % 64)
            if form == "off24":
                ml = max(ml, 16)
            if form == "rep":
                seqs.append((L, 4, off, "new16"))
                pos += len(L) + 4
                L = rnd.randbytes(j % 3)
            seqs.append((L, ml, off, form))
            pos += len(L) + ml
    return seqs


@functools.lru_cache(maxsize=None)
def match_vectors():
    """(name, block, plain, reference-comparable): one block per codeword form and offset range."""
    rnd = random.Random(4242)
    out = []
    for form in ("lz4", "new16", "rep", "off24"):
        for lo, hi in ((1, 8), (8, 521)):
            seqs = _match_seqs(rnd, range(lo, hi), form)
            last = rnd.randbytes(64)
            plain = model_decode(seqs, last)
            out.append(("%s offsets %d..%d" % (form, lo, hi - 1), encode(seqs, last, form == "lz4"), plain, lo >= 8))
    return out


@functools.lru_cache(maxsize=None)
def offset_edge_vectors():
    """(name, block, plain or None = must be refused, reference-comparable): a first match whose offset is op (accepted), op + 1 or
    0 (refused)."""
    rnd = random.Random(77)
    out = []
    for form in ("lz4", "new16", "off24"):
        for P in (1, 7, 8, 9, 64, 300):
            for off, ok in ((P, True), (P + 1, False), (0, False)):
                seqs = [(rnd.randbytes(P), 20, off, form)]
                last = rnd.randbytes(40)
                plain = model_decode(seqs, last)
                assert (plain is not None) == ok
                out.append(("%s op %d offset %d" % (form, P, off), encode(seqs, last, form == "lz4"), plain, ok and off >= 8))
    return out


def huf_max_bits(data, max_bits):
    """The longest code HUF_buildCTable gives `data` under the limit."""
    ref = util.reference()
    count = (C.c_uint * 256)()
    vals, cnts = np.unique(np.frombuffer(data, dtype=np.uint8), return_counts=True)
    for v, c in zip(vals, cnts):
        count[int(v)] = int(c)
    ctab = (C.c_uint * 256)()
    ref.HUF_buildCTable.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint]
    ref.HUF_buildCTable.restype = C.c_size_t
    return ref.HUF_buildCTable(ctab, count, int(vals[-1]), max_bits)


def huf_payload(data, max_bits=11):
    """huff0 4-stream payload of `data` from the reference encoder (HUF_compress2; below its size threshold HUF_buildCTable +
    HUF_writeCTable + HUF_compress4X_usingCTable), or None when it does not come out shorter than the data."""
    ref = util.reference()
    n = len(data)
    dst = C.create_string_buffer(2 * n + 1024)
    if n > 64:
        ref.HUF_compress2.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint, C.c_uint]
        ref.HUF_compress2.restype = C.c_size_t
        c = ref.HUF_compress2(dst, len(dst), data, n, 255, max_bits)
        return dst.raw[:c] if 1 < c < n else None
    count = (C.c_uint * 256)()
    for x in data:
        count[x] += 1
    msv = max(data)
    ctab = (C.c_uint * 256)()
    ref.HUF_buildCTable.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint]
    ref.HUF_buildCTable.restype = C.c_size_t
    ref.HUF_writeCTable.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_uint]
    ref.HUF_writeCTable.restype = C.c_size_t
    ref.HUF_compress4X_usingCTable.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    ref.HUF_compress4X_usingCTable.restype = C.c_size_t
    bits = ref.HUF_buildCTable(ctab, count, msv, max_bits)
    h = ref.HUF_writeCTable(dst, len(dst), ctab, msv, bits)
    if h == 0 or h > len(dst):
        return None
    c = ref.HUF_compress4X_usingCTable(C.addressof(dst) + h, len(dst) - h, data, n, ctab)
    if c == 0 or c > len(dst):
        return None
    return dst.raw[:h + c] if h + c < n else None


def _fib_data(rnd, n, nsym, order=None):
    """Fibonacci-like symbol counts (the deepest trees); order 'up' / 'down': the most frequent symbol has the highest / lowest value."""
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    syms = rnd.sample(range(256 if nsym > 8 else nsym), nsym)     # small alphabets of small values: the nibble weight header
    if order:
        syms = sorted(syms, reverse=order == "down")
    pool = b"".join(bytes([s]) * max(1, v * n // sum(f)) for s, v in zip(syms, f))
    return bytes(rnd.choice(pool) for _ in range(n)) if n < 4096 else bytes(np.random.default_rng(n).choice(np.frombuffer(pool, dtype=np.uint8), n))


def _alpha_data(rnd, n, nsym):
    syms = rnd.sample(range(256 if nsym > 8 else nsym), nsym)
    base = list(syms) + [syms[0]] * nsym * 3                     # every symbol present, one of them frequent
    out = bytearray(syms) if n >= nsym else bytearray()
    rng = np.random.default_rng(nsym * 1000 + n)
    out += bytes(np.array(base, dtype=np.uint8)[rng.integers(0, len(base), n - len(out))])
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def huf_vectors():
    """(name, block, plain): literal-only sub-blocks whose literals stream is huff0 from the reference encoder.  Also returns the
    set of weight-header forms that occurred ('nibble' / 'fse')."""
    rnd = random.Random(31)
    out, forms = [], set()
    cases = [("len%d alpha2" % n, _alpha_data(rnd, n, 2)) for n in range(12, 21)]
    cases += [("len%d fib4" % n, _fib_data(rnd, n, 4)) for n in range(12, 21)]
    for nsym in (2, 128, 129, 255, 256):
        for n in (4096 + 1, 4096 + 2, 4096 + 3, 4096 + 4, 131072):
            cases.append(("alpha%d len%d" % (nsym, n), _alpha_data(rnd, n, nsym)))
    # Fibonacci-like frequencies: the code lengths hit the limit (the Lizard writers use the default, 11).  At 12 bits the most
    # frequent symbol gets weight 12, which the format only allows for the last (implied) one: it has the highest value here
    # (weight_refusal_vectors has the other order).
    deep = [(nsym, 131072, 11) for nsym in (20, 40, 200)] + [(nsym, n, 12) for nsym in (15, 30) for n in (65536, 131072)]
    for nsym, n, bits in deep:
        data = _fib_data(rnd, n, nsym, "up" if bits == 12 else None)
        assert huf_max_bits(data, bits) == bits, (nsym, n, bits)
        cases.append(("fib%d len%d %d bits" % (nsym, n, bits), data, bits))
    for name, data, *bits in cases:
        p = huf_payload(data, *bits)
        if p is None:
            continue
        forms.add("nibble" if p[0] >= 128 else "fse")
        out.append((name, _container(30, b"", b"", lits_huf=(len(data), p)), data))
    return out, frozenset(forms)


def _nibble_header(weights):
    ws = list(weights) + [0] * (len(weights) & 1)
    return bytes([127 + len(weights)]) + bytes((ws[i] << 4) | ws[i + 1] for i in range(0, len(ws), 2))


@functools.lru_cache(maxsize=None)
def weight_refusal_vectors():
    """(name, block): nibble weight headers edited into each refusal case of lzd_read_weights_lane0 (lz_unpack.h:157-173),
    followed by a plausible jump table and bitstreams.  (An odd count of weight-1 symbols cannot be written: the weights sum to
    2^tableLog with the implied last one, and every weight above 1 adds an even number, so the count is always even.)"""
    body = struct.pack("<HHH", 2, 2, 2) + bytes([0x5A, 0x81, 0x3C, 0x81, 0x77, 0x82, 0x19, 0x84])
    cases = [
        ("weight 12", [12, 1, 1]),
        ("weight 15", [15, 2, 1]),
        ("table log 13", [11, 11, 11, 11]),
        ("table log 13, many", [10] * 8 + [1, 1]),
        ("remainder 3", [3, 1]),
        ("remainder 5", [4, 2, 1]),
        ("no weight-1 symbol", [2, 2, 2]),
        ("no weight-1 symbol, wide", [3, 3, 2, 2, 2, 2]),
        ("all weights zero", [0, 0, 0]),
    ]
    out = []
    for name, w in cases:
        p = _nibble_header(w) + body
        out.append((name, _container(30, b"", b"", lits_huf=(len(p) + 40, p))))
    # the reference encoder at 12 bits with the most frequent symbol first: an explicit weight 12 (its own decoder refuses it too)
    data = _fib_data(random.Random(12), 65536, 16, "down")
    assert huf_max_bits(data, 12) == 12
    out.append(("reference encoder, explicit weight 12", _container(30, b"", b"", lits_huf=(len(data), huf_payload(data, 12)))))
    return out


@functools.lru_cache(maxsize=None)
def long_offset_vectors():
    """(name, block, plain): raw sub-blocks (flag 128) of random bytes, then one LIZv1 sub-block whose 24-bit offsets reach 4 MiB + 1
    .. 16 MiB - 1 back (only levels 29 / 49 have that window, too slow to write multi-MiB blocks with)."""
    rnd = random.Random(16)
    head = bytes(np.random.default_rng(16).integers(0, 256, 16 << 20, dtype=np.uint8))
    raw = bytes([29])
    for at in range(0, len(head), 4 << 20):
        raw += bytes([128]) + _le24(4 << 20) + head[at:at + (4 << 20)]
    offs = [(4 << 20) + 1, (4 << 20) + 7, (4 << 20) + 4096, 5 << 20, (8 << 20) - 1, 8 << 20, (8 << 20) + 1, (12 << 20) + 12345,
            (16 << 20) - 65536, (16 << 20) - 2, (16 << 20) - 1]
    seqs = [(rnd.randbytes(rnd.randrange(0, 20)), rnd.choice([16, 17, 40, 46, 47, 48, 300, 70000]), off, "off24") for off in offs]
    seqs.append((rnd.randbytes(3), 20, 70000, "off24"))
    seqs.append((b"", 30, (4 << 20) + 3, "off24"))
    seqs.append((rnd.randbytes(5), 20, (4 << 20) + 3, "rep"))      # the repeat offset is the last 24-bit one
    last = rnd.randbytes(40)
    plain = model_decode(seqs, last, prefix=head)
    sub = encode(seqs, last, False)[1:]                            # (without its level byte)
    return [("offsets 4 MiB .. 16 MiB back", raw + sub, plain)]


# ---------------------------------------------------------------- the valid blocks the round trips do not reach -----------------

FAMILY_LEVELS_4M = [10, 31, 12, 37, 19, 40, 41, 45, 46, 49]       # fastSmall fast noChain hashChain optimalBT(LZ4) fastBig priceFast lowestPrice optimal optimalBT(LIZv1)
BIG_PRODUCT_LEVELS = [20, 21, 22, 40, 41, 42, 10, 13]


@functools.lru_cache(maxsize=None)
def valid_reference_blocks(with_4mib=True):
    """(name, block, plain): the reference at all 40 levels on a 4 KiB and a 256 KiB block, one 4 MiB block per parser family."""
    rnd = random.Random(404)
    d4k, d256k = _sample(rnd, 4096), util.datagen(262144, 0.6, 0.0, 55)
    out = []
    for lv in REF_LEVELS:
        out.append(("ref L%d 4 KiB" % lv, _ref_compress(d4k, lv), d4k))
        out.append(("ref L%d 256 KiB" % lv, _ref_compress(d256k, lv), d256k))
    if with_4mib:
        d4m = util.datagen(3 << 20, 0.5, 0.0, 56) + bytes(70000) + util.datagen((1 << 20) - 70000, 0.3, 0.0, 57)
        for lv in FAMILY_LEVELS_4M:
            out.append(("ref L%d 4 MiB" % lv, _ref_compress(d4m, lv), d4m))
    return out


def big_product_data():
    return util.datagen((5 << 20) + 123, 0.5, 0.0, 31) + bytes(300000) + util.datagen(1 << 20, 0.2, 0.0, 32)


# ---------------------------------------------------------------- shared checks -------------------------------------------------

def check_vectors(vectors, run, ref_check):
    """(name, block, plain or None, compare-with-reference) through the guarded runner at cap = len(plain) (and len - 1, which
    must be refused) and the host decoder; refusals where plain is None."""
    items = []
    for name, block, plain, _ in vectors:
        cap = len(plain) if plain is not None else 4096
        items.append((block, cap))
        if plain is not None and len(plain) > 1:
            items.append((block, cap - 1))
    res = guarded_decode(items, run)
    k = 0
    for name, block, plain, cmp_ref in vectors:
        r, out = res[k]
        k += 1
        hr, hout = host_decode(block, len(plain) if plain is not None else 4096)
        if plain is None:
            assert r == ERR and hr == ERR, "%s: must be refused (wave %s, host %s)" % (name, r, hr)
            continue
        assert r == len(plain) and out == plain, "%s: wave decoder %s, want %d bytes" % (name, r, len(plain))
        assert hr == len(plain) and hout == plain, "%s: host decoder %s" % (name, hr)
        if len(plain) > 1:
            assert res[k][0] == ERR, "%s: accepted into one byte less than it decodes to" % name
            assert host_decode(block, len(plain) - 1)[0] == ERR, name
            k += 1
        if cmp_ref and ref_check:
            rr, rout = ref_decode(block, len(plain))
            assert rr == len(plain) and rout == plain, "%s: the reference decoder %s" % (name, rr)
    return res


def hand_built_vectors():
    v = [(n, b, p, ref_ok) for n, b, p, ref_ok in match_vectors()]
    v += list(offset_edge_vectors())
    hv, forms = huf_vectors()
    assert forms == {"nibble", "fse"}, forms
    assert len(hv) >= 40
    v += [(n, b, p, True) for n, b, p in hv]
    v += [(n, b, None, False) for n, b in weight_refusal_vectors()]
    v += [(n, b, p, True) for n, b, p in long_offset_vectors()]
    return v


def _oracle_compress(data, level):
    return util.oracle_compress(data, level)


# ---------------------------------------------------------------- CPU: the emulator twin --------------------------------------

def test_model_matches_reference_decoder():
    """The model and the hand-built encoder agree with the reference decoder wherever its semantics are the product's (offsets >= 8)."""
    need_reference()
    n = 0
    for name, block, plain, ref_ok in match_vectors():
        if ref_ok:
            assert ref_decode(block, len(plain)) == (len(plain), plain), name
            n += 1
    for name, block, plain in huf_vectors()[0]:
        assert ref_decode(block, len(plain)) == (len(plain), plain), name
        n += 1
    assert n >= 40


def test_emulated_decoder_hand_built_vectors():
    need_reference()
    check_vectors(hand_built_vectors(), _emul_run, ref_check=True)


def test_emulated_decoder_valid_reference_blocks():
    """The reference at all 40 levels, 4 KiB and 256 KiB (the 4 MiB blocks and the product's > 4 MiB blocks: GPU only, the emulated
    wave takes minutes on them)."""
    need_reference()
    check_vectors([(n, b, p, True) for n, b, p in valid_reference_blocks(with_4mib=False)], _emul_run, ref_check=True)


def test_emulated_decoder_differential_fuzz():
    """At least 3 000 damaged blocks from all 40 reference levels and the product's levels: the emulated wave decoder equals the
    host decoder on every one, under every guard."""
    need_reference()
    items = fuzz_cases(SEED, [9, 150, 1200, 6000], 6, REF_LEVELS, [10, 21, 30, 41, 13, 36, 20, 22], _oracle_compress)
    results = guarded_decode([(b, cap) for b, cap, _, _ in items], _emul_run)
    cnt = check_differential(items, results)
    print("emulator differential (seed %d): %s" % (SEED, cnt))
    assert cnt["damaged"] >= 3000 and cnt["accepted"] > 0 and cnt["refused"] > 0


def test_walker_reaches_every_field():
    """The structured damage has something to hit: reference blocks with huff0 streams expose every field kind."""
    need_reference()
    data = util.datagen(100000, 0.5, 0.0, 3)
    kinds = set()
    for lv in (30, 41, 49, 39):
        f = walk(_ref_compress(data, lv))
        kinds |= {k for k, v in f.items() if v}
    assert kinds == {"flag", "len", "huf_n", "huf_c", "hdr", "jump", "end"}, kinds


# ---------------------------------------------------------------- GPU ------------------------------------------------------------

def _product_gpu_compress(data, level):
    out, r = util.compress_with(product_lib().Lizard_compress, data, level)
    assert r > 0, (level, len(data))
    return out


def _host_form_and_one_block(items, results):
    """The same batch through the packed host form (same results) and a sample through LizardGPU_decompress_safe."""
    hf = host_form_decode(items)
    for i, (a, b) in enumerate(zip(results, hf)):
        assert a == b, "item %d: device form %s, host form %s (seed %d)" % (i, a[0], b[0], SEED)
    L = product_lib()
    for i in random.Random(SEED).sample(range(len(items)), min(200, len(items))):
        block, cap = items[i]
        dst = C.create_string_buffer(cap + 64)
        r = L.LizardGPU_decompress_safe(block, dst, len(block), cap)
        want = results[i][0]
        assert (r < 0) if want == ERR else (r == want and dst.raw[:r] == results[i][1]), "item %d: one-block entry %d" % (i, r)


@pytest.mark.gpu
def test_gpu_decoder_hand_built_vectors():
    need_reference()
    vecs = hand_built_vectors()
    res = check_vectors(vecs, _device_run, ref_check=True)
    items = []
    for name, block, plain, _ in vecs:
        cap = len(plain) if plain is not None else 4096
        items.append((block, cap))
        if plain is not None and len(plain) > 1:
            items.append((block, cap - 1))
    _host_form_and_one_block(items, res)


@pytest.mark.gpu
def test_gpu_decoder_valid_blocks_beyond_the_round_trips():
    need_reference()
    vecs = [(n, b, p, True) for n, b, p in valid_reference_blocks()]
    data = big_product_data()
    for lv in BIG_PRODUCT_LEVELS:
        comp = _product_gpu_compress(data, lv)
        assert comp == util.oracle_compress(data, lv), lv
        vecs.append(("product L%d %d bytes" % (lv, len(data)), comp, data, True))
    check_vectors(vecs, _device_run, ref_check=True)


@pytest.mark.gpu
def test_gpu_decoder_differential_fuzz():
    """At least 20 000 damaged blocks (reference at all 40 levels, the product's GPU compressor at its 23) mixed with intact ones in
    the same launches: every result equal to the host decoder's, every guard intact, both read patterns identical, the packed
    host form identical."""
    need_reference()
    L = product_lib()
    levels = [lv for lv in GPU_LEVELS if L.LizardGPU_levelSupported(lv)]
    assert len(levels) == 23
    items = fuzz_cases(SEED, [5, 40, 700, 4096, 16384], 16, REF_LEVELS, levels, _product_gpu_compress)
    items += fuzz_cases(SEED + 1, [70000, 262144], 2, REF_LEVELS, levels, _product_gpu_compress)
    pairs = [(b, cap) for b, cap, _, _ in items]
    results = guarded_decode(pairs, _device_run)
    cnt = check_differential(items, results, twin=emul_decode)
    _host_form_and_one_block(pairs, results)
    print("GPU differential (seed %d): %s" % (SEED, cnt))
    assert cnt["damaged"] >= 20000 and cnt["accepted"] > 0 and cnt["refused"] > 0
