"""Inputs of tests/test_huf_stream_emul.py and tests/test_huf_stream_gpu.py: named byte streams for lz_put_stream_huf
(lizard_amd/csrc/lz_huf.h) on its own, each built for one path of the stage, and the bytes the stage must write for them.

A stream is a count vector spread over symbols (np.repeat) and shuffled with a seed of its own, so the whole set is the same on
every machine.  The families, and the path each one is there for (the LZ_STAT marks of lz_huf.h, see MARKS):

  raw_*        n <= 1024: Lizard_writeStream stores them raw before the stage looks at a byte; border_* (1025..1028, a skewed
               alphabet) enter the stage, build a tree, and still come out raw — no payload can save 512 bytes there.
               n = 0 is absent: lz_write_subblock_seq (lz_block.h) reaches the stage only for a sub-block with at least one
               sequence, whose flag stream holds a token per sequence and whose literal stream holds the last literals.
  rle_*        one symbol
  uniform      all 256 symbols alike: "not compressible" before any tree is built
  geo_*        sizes around the histogram's and the packer's step sizes (4 x 256 bytes, 1 024 symbols, segments of (n + 3) / 4
               bytes; 4097, 4099, 8193, 16385: a last lane group of fewer than 16 symbols); 131072 is HUF_BLOCKSIZE_MAX
  fib_*        Fibonacci counts: a tree deeper than 11, lz_huf_set_max_height cuts and repays
  merge_*      64 .. 256 symbols: the merge's three register cursors cross their 64-entry chunks
  ones_*       hundreds of leaves of count 1 under a few heavy ones
  hdr_*        two and four symbols far apart (FSE weight header with zero runs in its NCount), symbols 0 / 1 (nibble header),
               a 13-symbol stream whose weight counts go through FSE_normalizeM2, and eq192: 192 symbols of one weight under
               symbol 192 with a quarter of the stream — HUF_compressWeights answers 1 ("one weight"), no nibble header exists
               for more than 128 symbols, HUF_writeCTable fails (huf_compress.c:158) and the stream stays raw
  negloop      a 128-symbol vector whose cut over-pays: the limiter's totalCost < 0 loop, also with rankLast[1] empty
  fate_*       two streams whose acceptance the three bytes of slack decide (test_emulator.py), one on each side of the flip
  rnd*         250 count vectors of five kinds over alphabets of 3 .. 256 symbols
"""
import ctypes
import functools
import random

import numpy as np

import util

HUF_BLOCKSIZE_MAX = 131072       # the reference's HUF_compress refuses more; the container's sub-blocks are no longer
MIN_HUF = 1024                   # Lizard_writeStream, lizard_compress.c:143: at most this many bytes are stored raw unseen

# LZ_STAT indices of lizard_amd/csrc/lz_huf.h
MARKS = {
    "rle": 13, "raw_exit": 14, "limiter": 15, "limiter_repay_pos": 16, "limiter_repay_neg": 17, "limiter_neg_rank1_empty": 18,
    "merge_general_step": 29, "merge_node_register_rolls": 30, "hdr_fse": 31, "hdr_nibbles": 36, "hdr_weights_error": 53,
    "hdr_no_nibbles_above_128": 56, "fse_normalize_early": 57, "fse_normalize_m2": 58, "pack_partial_group": 59,
    "exact_sizes": 60, "pack": 61,
}


def from_counts(counts, seed, symbols=None):
    """counts[i] bytes of symbols[i] (default: i), shuffled."""
    counts = np.asarray(counts, dtype=np.int64)
    symbols = np.arange(len(counts)) if symbols is None else np.asarray(symbols)
    d = np.repeat(symbols.astype(np.uint8), counts)
    np.random.RandomState(seed).shuffle(d)
    return d.tobytes()


def _geo_bytes(n, seed):
    return np.minimum(np.random.RandomState(seed).geometric(0.2, n), 255).astype(np.uint8).tobytes()


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def merge_counts(k):
    return [max(1, int(3000 * 0.97 ** i)) for i in range(k)]


def fate_stream(m, n=6000, seed=1):
    """m incompressible bytes in front of 16-symbol bytes (test_emulated_huffman_streams_whose_fate_three_bytes_decide)."""
    rs = np.random.RandomState(seed)
    hi_part, lo_part = rs.randint(0, 256, n).astype(np.uint8), rs.randint(0, 16, n).astype(np.uint8)
    return np.concatenate([hi_part[:m], lo_part[m:]]).tobytes()


FATE_M = (2370, 2371)            # the last m that is accepted and the first that is stored raw; both go through the exact pass (mark 60)

# FSE_normalizeM2 for the weights of symbols 0 .. 11: eight code lengths that occur once and two that occur twice give the weight
# counts 1 x 8, 2 x 2 of 12; at tableLog 5 those round to 3 x 8 + 5 x 2 = 34 of 32 slots, and the 2 too many are not less than
# half of the largest share (fse_compress.c:617).  Lengths 1 .. 8, 10, 10, 11, 11 and 10 for symbol 12 (which has no weight in the
# header) fill the code space exactly: counts 2^(11 - length) x 4.  n = 8192, so that HUF_optimalTableLog allows 11 bits.
M2_COUNTS = [4 << (11 - length) for length in (1, 2, 3, 4, 5, 6, 7, 8, 10, 10, 11, 11, 10)]

NEGLOOP_SEED = 1434              # random_vector(.., kind 0, 128 symbols, about 7 900 bytes): the first seed that reaches marks 17 and 18

# What a stream is in the set for: (prefix of its name, marks it must reach on its own).  tests/test_huf_stream_emul.py checks it.
REACHES = (
    ("border_", ("raw_exit",)), ("rle_", ("rle",)), ("uniform_", ("raw_exit",)), ("geo_", ("pack",)),
    ("geo_4097", ("pack_partial_group",)), ("geo_4099", ("pack_partial_group",)), ("geo_8193", ("pack_partial_group",)),
    ("geo_16385", ("pack_partial_group",)), ("fib_", ("limiter", "limiter_repay_pos", "pack")), ("merge_", ("merge_general_step", "pack")),
    ("merge_65", ("merge_node_register_rolls",)), ("merge_1", ("merge_node_register_rolls",)), ("merge_2", ("merge_node_register_rolls",)),
    ("ones_", ("merge_general_step", "merge_node_register_rolls", "hdr_fse", "pack")), ("hdr_nibbles_", ("hdr_nibbles", "pack")),
    ("hdr_fse_", ("hdr_fse", "fse_normalize_early", "pack")), ("hdr_eq192", ("hdr_no_nibbles_above_128", "raw_exit")),
    ("hdr_m2", ("fse_normalize_m2", "pack")), ("negloop", ("limiter_repay_neg", "limiter_neg_rank1_empty", "pack")),
    ("fate_accepted", ("exact_sizes", "pack")), ("fate_raw", ("exact_sizes", "raw_exit")),
)

KINDS = ("geometric", "small_plus_large", "fib_head_flat_tail", "powers_of_two", "flat_plus_large")


def scale_counts(c, target=None):
    """Counts brought to 1024 < sum <= 131072 (to about `target` when given), every symbol kept."""
    c = np.maximum(np.asarray(c, dtype=np.float64), 1.0)
    total = c.sum()
    want = total if target is None else float(target)
    want = min(max(want, MIN_HUF + 64.0 + len(c)), HUF_BLOCKSIZE_MAX - len(c))
    out = np.maximum((c * (want / total)).astype(np.int64), 1)
    while out.sum() > HUF_BLOCKSIZE_MAX:
        out[out.argmax()] -= out.sum() - HUF_BLOCKSIZE_MAX
    while out.sum() <= MIN_HUF:
        out[out.argmax()] += MIN_HUF + 1 - out.sum()
    return out


def random_vector(seed, kind=None, k=None, target=None):
    """(counts, symbols) of one of the five KINDS; the counts land on the symbols in random order."""
    r = random.Random(seed)
    kind = r.randrange(5) if kind is None else kind
    k = r.randrange(3, 257) if k is None else k
    if kind == 0:
        ratio, top = r.uniform(0.5, 0.99), r.uniform(50, 60000)
        c = [max(1.0, top * ratio ** i) for i in range(k)]
    elif kind == 1:
        c = [r.randrange(1, 5) for _ in range(k)]
        c[0] = r.randrange(200, 100000)
    elif kind == 2:
        h = min(k, r.randrange(8, 24))
        c = _fib(h)[::-1] + [r.randrange(1, 40)] * (k - h)
    elif kind == 3:
        c = [1 << r.randrange(0, 13) for _ in range(k)]
    else:
        c = [r.randrange(1, 300)] * k
        c[0] = c[0] * r.randrange(4, 400)
    if target is None and r.random() < 0.7:
        target = int(2 ** r.uniform(10.2, 17))
    counts = scale_counts(c, target)
    order = list(range(k))
    r.shuffle(order)
    counts = counts[order]
    symbols = np.array(sorted(r.sample(range(256), k)))
    return counts, symbols


@functools.lru_cache(maxsize=None)
def streams():
    """((name, bytes), ...)"""
    out = []
    for n in (1, 3, 4, 5, 255, 1023, 1024):
        out.append(("raw_%d" % n, _geo_bytes(n, 100 + n)))
    for n in (1025, 1026, 1027, 1028):
        out.append(("border_%d" % n, _geo_bytes(n, 100 + n)))
    out += [("rle_1025", b"\x07" * 1025), ("rle_5000", b"\xfe" * 5000)]
    out.append(("uniform_20000", np.random.RandomState(7).randint(0, 256, 20000).astype(np.uint8).tobytes()))
    for n in (2047, 2048, 2049, 4095, 4096, 4097, 4099, 5121, 8193, 16385, 65537, 131071, 131072):
        out.append(("geo_%d" % n, _geo_bytes(n, n)))
    for k in (16, 18, 20, 22, 24):
        out.append(("fib_%d" % k, from_counts(_fib(k), 200 + k)))
    for k in (64, 65, 128, 129, 130, 192, 193, 255, 256):
        out.append(("merge_%d" % k, from_counts(merge_counts(k), 300 + k)))
    out.append(("ones_200_pow2", from_counts([1] * 200 + [1 << i for i in range(14)], 401)))
    out.append(("ones_250_big", from_counts([1] * 250 + [40000], 402)))
    out.append(("hdr_nibbles_0_1", from_counts([3000, 1001], 501)))
    out.append(("hdr_fse_0_255", from_counts([3000, 1001], 502, symbols=[0, 255])))
    out.append(("hdr_fse_0_85_170_255", from_counts([2500, 900, 400, 201], 503, symbols=[0, 85, 170, 255])))
    out.append(("hdr_eq192", from_counts([10] * 192 + [630], 504)))
    out.append(("hdr_m2", from_counts(M2_COUNTS, 505)))
    c, s = random_vector(NEGLOOP_SEED, kind=0, k=128, target=7900)
    out.append(("negloop", from_counts(c, 506, s)))
    out.append(("fate_accepted", fate_stream(FATE_M[0])))
    out.append(("fate_raw", fate_stream(FATE_M[1])))
    for i in range(250):
        c, s = random_vector(1000 + i, kind=i % 5)
        out.append(("rnd%03d_%s" % (i, KINDS[i % 5]), from_counts(c, 2000 + i, s)))
    names = [name for name, _ in out]
    assert len(set(names)) == len(names)
    assert all(1 <= len(d) <= HUF_BLOCKSIZE_MAX for _, d in out)
    return tuple(out)


def want_of(data):
    """(bytes, huffed) of Lizard_writeStream for a Huffman candidate (lizard_compress.c:141-183), with the oracle's HUF_compress
    (pinned to the compiled reference by tests/test_oracle.py)."""
    n = len(data)
    hdr = bytes([n & 255, (n >> 8) & 255, n >> 16])
    if n > MIN_HUF:
        cap = n + (n >> 8) + 8 + 129 + 64
        tmp = ctypes.create_string_buffer(cap)
        c = util.oracle().lzo_huf_compress(tmp, cap, data, n)
        if c != 0 and c < (1 << 63) and c + c // 8 + 512 < n:       # (an error code is a size_t just below 2^64)
            return hdr + bytes([c & 255, (c >> 8) & 255, c >> 16]) + tmp.raw[:c], 1
    return hdr + data, 0


@functools.lru_cache(maxsize=None)
def expected():
    """name -> (bytes, huffed); computed once and shared."""
    return {name: want_of(data) for name, data in streams()}


def write_case_file(path):
    """The set for tests/huf_stream_kernels: 'HUFS', u32 count, then per stream u32 length of the name, u32 n, u32 size of the
    expected bytes, u32 huffed, the name, the stream, the expected bytes (little-endian, no padding).  Returns the number of streams."""
    import struct
    want = expected()
    with open(path, "wb") as f:
        f.write(b"HUFS" + struct.pack("<I", len(streams())))
        for name, data in streams():
            w, h = want[name]
            f.write(struct.pack("<IIII", len(name), len(data), len(w), h) + name.encode() + data + w)
    return len(streams())
