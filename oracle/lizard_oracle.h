/*
 * oracle/lizard_oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * Plain-C, single-threaded restatement of the Lizard block-compress path (reference inikep/lizard 1.0,
 * 64-bit build), written from the behaviour of the reference, not from its text. It is the checker
 * for the HIP path: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it.
 * The product library (lizard_amd/csrc) never links, calls or falls back to anything in oracle/.
 *
 * Parity status: PINNED — tests/test_oracle.py checks this restatement (a) against the known-answer
 * sums/XXH64 chains recorded from the compiled reference (tests/golden/) and (b), when
 * oracle/_ref/ is present, byte-for-byte against the unmodified reference library built with
 * -DLIZARD_RESET_MEM (zero-initialised match-finder state, reference lib/lizard_compress.c:329-332).
 *
 * Oracle definition: per-block output of Lizard_compress_extState() on a zero-filled
 * state.  Supported levels: 10, 11, 30, 31 (fastSmall / fast + fastLZ4 codewords), 13..17, 34..38 (hashChain +
 * fastLZ4 codewords), 12, 32, 33 (noChain + fastLZ4 codewords), 20, 40 (fastBig + LIZv1 codewords), 21, 22, 41, 42 (priceFast + LIZv1 codewords); levels >= 30
 * add the huff0 stage.
 */
#ifndef LIZARD_ORACLE_H
#define LIZARD_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Lizard_compressBound (reference lib/lizard_compress.h:124). */
int lzo_compress_bound(int srcSize);

/* 1 if this oracle restates `level`, else 0. */
int lzo_level_supported(int level);

/* Lizard_compress_extState on a zero-filled state (reference lib/lizard_compress.c:583-593,472-547).
 * Returns bytes written to dst, 0 on failure (dst too small, unsupported level/size). */
int lzo_compress(const void* src, void* dst, int srcSize, int dstCapacity, int level);

/* HUF_compress (reference lib/entropy/huf_compress.c:609): returns compressed size, 0 if not
 * compressible, 1 for single-symbol RLE, or (size_t)-1 for the error cases that the caller treats as
 * "store raw". */
size_t lzo_huf_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize);

/* Test-only: the state of the hashChain / noChain match finder (levels 12-17, 32-38) as a function of the block's bytes, from
 * this file's restatements of Lizard_Insert(NoChain) and Lizard_InsertAndFindBestMatch(NoChain) driven on ONE context at ascending
 * positions p = 0 .. nIns - 1, nIns = n >= 8 ? n - 7 : 0 — the sequential model the chain build of the product's kernels
 * (lz_hc_build, lz_hc_hits_plain, lz_hc_hits) is compared with.  Per position:
 *   prev[p]      distance from p to the head of p's bucket at the moment the insert reaches p; 0 = empty bucket or farther than
 *                65535 (exactly 65535 stays); the head moves only when p - head >= MIN_OFFSET (hashchain.h:38, nochain.h:20)
 *   two[p]       prev[p] | s << 16, s = prev[p] + prev[p - prev[p]] when both links exist and the sum is <= 65535, else 0
 *   hit[p]       1 when the first search at p returns a length above 0
 *   first[p]     (may be NULL) length | offset << 16 of that search under the limit the parse passes at p (the end of p's 128 KiB
 *                sub-block or of the block, minus LASTLITERALS); 0 = nothing found, or the parse never searches at p (p at or
 *                beyond the sub-block's mflimit).  Exact where the length is at most 16; a longer match is reported with length 17
 *                (the model cuts the limit to p + 17: a run would cost n^2 * searchNum compares otherwise), and mayBeOpen[p] is 1
 *                at every such position (checked: -2 is returned if not)
 *   mayBeOpen[p] (may be NULL) 1 when lz_hc_hits may leave the first search at p to the parse: one of the first four in-window
 *                chain candidates agrees with p in all the bytes that pass compares (16, or 8 when p + 16 > n) and the limit
 *                leaves room for more, or the chain has a fifth in-window candidate within searchNum
 * Returns nIns, -1 for a level without these parsers (first / mayBeOpen are filled together or not at all). */
int lzo_hc_tables(const void* src, int n, int level, uint16_t* prev, uint32_t* two, uint8_t* hit, uint32_t* first, uint8_t* mayBeOpen);

/* Test-only: number of searches (both kinds, hashChain and noChain) since the last reset that arrived at a position below
 * nextToUpdate; reset != 0 clears the counter. */
unsigned long long lzo_searches_below_next_to_update(int reset);

/* RDG_genBuffer (reference programs/datagen.c:153): deterministic synthetic data. */
void lzo_datagen(void* buffer, size_t size, double matchProba, double litProba, unsigned seed);

#ifdef __cplusplus
}
#endif
#endif
