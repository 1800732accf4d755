"""Named inputs for the chain build of the hashChain / noChain levels (lz_hc_build, lz_hc_hits_plain, lz_hc_hits in
lizard_amd/csrc/lz_hashchain.h), shared by tests/test_hc_build_emul.py (CPU: the kernels on the SIMT emulator) and
tests/test_hc_build_gpu.py (the same inputs through tests/hc_build_kernels.hip on the device).  No test in here.

Every case is built for one edge of the build — nIns = n - 7 around a step of 64 positions, a group of 8 steps, the 16-step queue of
pass 2, a 2^14-position window and a 2^18-position segment; one bin that holds every position; links on both sides of MIN_OFFSET; a
link of exactly 65535 and of 65536; two links that sum to 65535 and to 65536; a link across a segment border; bins that are empty in
the first segment; a bucket last seen more than 65535 back across a segment border — and is as small as that edge allows.

VARIANTS: the forms the library instantiates, (name, searchLength, hashLog, searchNum, pre, oracle level of the model, small only).
pre = the pass is lz_hc_hits (levels 16 / 17 / 37 / 38) instead of lz_hc_hits_plain.
"""
import functools
import random
import struct

import util

SEG = 1 << 18
SMALL = 1 << 16                   # "small" cases: searchNum 8 and 256 run on these only

VARIANTS = (
    ("h5_18_n1", 5, 18, 1, 0, 12, False),
    ("h5_18_n2", 5, 18, 2, 0, 13, False),
    ("h5_18_n8", 5, 18, 8, 0, 15, True),
    ("h4_18_n16", 4, 18, 16, 1, 16, False),
    ("h4_18_n256", 4, 18, 256, 1, 17, True),
    ("h5_14_n1", 5, 14, 1, 0, 32, False),
)

# LZ_HC_MARK marks of lz_hc_build (lz_hashchain.h names them)
MARKS = {"scalar_replay": 0, "step_straddles_bins": 1, "bin_left_fresh": 2, "heads_stored": 3, "heads_loaded": 4,
         "pass3_more_loop": 5, "trailing_bin_fresh": 6}
MARK_COUNT = 7


def _period(per, n, seed):
    pat = random.Random(seed).randbytes(per)
    return (pat * (n // per + 1))[:n]


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, data, has_repeat)]; has_repeat: the case is built to hold a position with a candidate at least MIN_OFFSET back that
    agrees in 4 bytes and that lz_hc_hits must decide, so the first-search table of the pre variants holds a decided non-zero entry."""
    out = []
    for n in (0, 7, 8, 9, 70, 71, 72, 518, 519, 520, 1030, 1031, 1032, 16390, 16391, 16392):
        out.append(("size_%d" % n, util.datagen(n, 0.5, 0.0, n + 3), n >= 16390))
    for name, n in (("seg_minus_1", SEG + 6), ("seg_exact", SEG + 7), ("seg_plus_1", SEG + 8), ("seg_plus_step", SEG + 71), ("three_segs", 2 * SEG + 8)):
        out.append((name, util.datagen(n, 0.5, 0.0, n + 3), True))
    for tag, n in (("40k", 40000), ("seg", SEG + 5000)):
        # (runs and short periods: every position but the first few has five candidates in the window, so lz_hc_hits may leave
        # all of them open — no decided non-zero entry is owed)
        out.append(("const_" + tag, b"\x5a" * n, False))
        for per in (2, 3, 7, 8, 9, 64):
            out.append(("period%d_%s" % (per, tag), _period(per, n, per), False))
        rng = random.Random(n)
        out.append(("two_letters_" + tag, bytes(rng.choice(b"ab") for _ in range(n)), True))
    # a 600-byte chunk in noise, again `dist` bytes later
    for dist in (65534, 65535, 65536, 65537):
        rng = random.Random(dist)
        chunk = rng.randbytes(600)
        buf = bytearray(rng.randbytes(dist + 600 + 100 + 300))
        buf[300:900] = chunk
        buf[300 + dist:900 + dist] = chunk
        out.append(("chunk_dist_%d" % dist, bytes(buf), dist <= 65535))
    # the chunk three times: the two links of the third copy sum to 65535 / 65536
    for total in (65535, 65536):
        rng = random.Random(total + 1)
        chunk = rng.randbytes(600)
        g1 = 30000
        buf = bytearray(rng.randbytes(200 + total + 600 + 100))
        for at in (200, 200 + g1, 200 + total):
            buf[at:at + 600] = chunk
        out.append(("chunk_two_links_%d" % total, bytes(buf), True))
    # a link across the segment border (a 300-byte chunk that ends at 2^18 and starts again at 2^18 + 50): the heads come out of hc.heads
    rng = random.Random(7)
    chunk = rng.randbytes(300)
    buf = bytearray(rng.randbytes(SEG + 50 + 300 + 200))
    buf[SEG - 300:SEG] = chunk
    buf[SEG + 50:SEG + 350] = chunk
    out.append(("chunk_across_segments", bytes(buf), True))
    # most bins are empty in segment 0 and first used in segment 1
    out.append(("period9_then_noise", _period(9, SEG + 7, 9) + random.Random(9).randbytes(5000), False))
    # a bucket last seen more than 65535 back, across a segment border: link 0
    rng = random.Random(10)
    first = rng.randbytes(SEG)
    out.append(("noise_then_copy_of_start", first + first[:1000] + rng.randbytes(100), False))
    return out


def jobs():
    """(case index, variant index) of every run."""
    C = cases()
    return [(ci, vi) for ci, (_, d, _) in enumerate(C) for vi, v in enumerate(VARIANTS) if not (v[6] and len(d) > SMALL)]


def total_bytes():
    return sum(len(d) for _, d, _ in cases())


def write_case_file(path):
    """'HCBI', case count, job count; per case: name length, n, has_repeat, name, bytes; per job: case index, variant index,
    searchLength, hashLog, searchNum, pre, oracle level.  Returns the number of jobs."""
    C, J = cases(), jobs()
    with open(path, "wb") as f:
        f.write(b"HCBI" + struct.pack("<II", len(C), len(J)))
        for name, data, rep in C:
            nb = name.encode()
            f.write(struct.pack("<III", len(nb), len(data), 1 if rep else 0) + nb + data)
        for ci, vi in J:
            _, sl, hl, sn, pre, level, _ = VARIANTS[vi]
            f.write(struct.pack("<7I", ci, vi, sl, hl, sn, pre, level))
    return len(J)
