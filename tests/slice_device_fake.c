/* tests/slice_device_fake.c — TEST INFRASTRUCTURE: lizard_amd/csrc/lizard_slice_device.c (LizardGPU_decompressFrameRanges_device: a count
 * pass and a fill pass over a batch of frames, two host waits, of which only the records that cover the caller's byte ranges are
 * decoded; LizardGPU_joinPlanesRange_device) compiled as a unit under test on a CPU, on the fake HIP runtime with DEFERRED streams.
 * Linked with tests/unframes_device_fake.c (the sequential model of lz_unframes_walk_kernel — the real walk on the emulator — which this
 * unit launches unchanged), tests/pipeline_fake.c (the context, the single-frame entry LizardGPU_decompressFrame_device on the same fake,
 * the emulator's record decoder) and tests/fake_hip.c as they are; this file adds plain sequential models of the unit's own launches:
 * lz_unslice_kernel (the emulator's record decoder, picks in a shuffled order) and lz_planes_range_kernel (the layout, bit by bit),
 * which check that everything they touch lies in live device memory.
 * sdf_run runs one call over caller-given frames and ranges and compares every range of every answered frame with the FULL decode of
 * LizardGPU_decompressFrame_device on the same fake; sdf_frame / sdf_flushed_frame make the frames of the tests.
 *   library : -shared (tests/test_slice_decompress_fake_device.py drives it through ctypes)
 *   program : -DSLICE_DEVICE_FAKE_MAIN, for the sanitizer build; exit 0 = all good */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../lizard_amd/csrc/lizard_slice_device.c"          /* unit under test, compiled into this harness */
#include "device_fake_common.h"
#include "lizard_oracle.h"

unsigned emul_unframe_record(const void* payload, unsigned size, unsigned word, void* slot, unsigned cap, unsigned seed);      /* tests/pipeline_fake_emul.cpp */

static unsigned long long g_launches[2];                      /* lzk_unslice_launch, lzk_planes_range_launch: since process start */
unsigned long long sdf_launches(int kind) { return g_launches[kind & 1]; }

/* ---- lz_unslice_kernel: one wave per pick, in whatever order the waves claim them ---- */
typedef struct { const LzUnframesEntry* frames; const uint64_t* offs; const uint32_t* words; const LzSlicePick* picks; uint8_t* dst; uint32_t* out; size_t n; } UnsliceK;
static void unslice_kernel(void* a)
{
    const UnsliceK* k = (const UnsliceK*)a;
    uint32_t* order;
    size_t i;
    if (!fh_check_dev(k->picks, k->n * sizeof *k->picks, "unslice: the picks") || !fh_check_dev(k->out, 4 * k->n, "unslice: results")) return;
    order = (uint32_t*)malloc(k->n * sizeof *order);
    dfc_shuffled(order, k->n);
    for (i = 0; i < k->n; i++) {
        const uint32_t b = order[i];
        const LzSlicePick* p = k->picks + b;
        const LzUnframesEntry* e = k->frames + p->frame;
        uint32_t word, size, r = 0xFFFFFFFFu;
        if (!fh_check_dev(e, sizeof *e, "unslice: a pick's frame entry")) continue;
        if (!fh_check_dev(k->offs + p->rec, 8, "unslice: a pick's payload offset") || !fh_check_dev(k->words + p->rec, 4, "unslice: a pick's word")) continue;
        word = k->words[p->rec]; size = word & 0x7FFFFFFFu;
        if (!fh_check_dev(k->dst + p->dstOff, e->maxBlock, "unslice: a pick's slot in d_dst")) continue;
        if (size && size <= e->maxBlock) {
            if (k->offs[p->rec] + size > e->srcSize || !fh_check_dev((const uint8_t*)(uintptr_t)e->src + k->offs[p->rec], size, "unslice: a pick's payload")) continue;
            r = emul_unframe_record((const uint8_t*)(uintptr_t)e->src + k->offs[p->rec], size, word, k->dst + p->dstOff, e->maxBlock, fh_rand() | 1u);
        }
        k->out[b] = r;
    }
    free(order);
}
int lzk_unslice_launch(LzCtx* c, const LzUnframesEntry* d_frames, const uint64_t* d_offs, const uint32_t* d_words, const LzSlicePick* d_picks, void* d_dst,
                       uint32_t* d_out, size_t nPicks, hipStream_t stream)
{
    UnsliceK k;
    if (!d_frames || !d_offs || !d_words || !d_picks || !d_dst || !d_out || nPicks == 0 || nPicks > 0xFFFFFFFFu) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_unslice_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    g_launches[0]++;
    k.frames = d_frames; k.offs = d_offs; k.words = d_words; k.picks = d_picks; k.dst = (uint8_t*)d_dst; k.out = d_out; k.n = nPicks;
    c->hostKernelMs = -1.0f;
    return fh_enqueue_kernel(stream, unslice_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- lz_planes_range_kernel: the layout of include/lizard_amd.h Part 3c / 3d, element by element ---- */
typedef struct { const LzPlanesRangeEntry* tab; uint32_t n; const uint64_t* pieces; } RangeK;
static void range_kernel(void* a)
{
    const RangeK* k = (const RangeK*)a;
    uint32_t t;
    if (!fh_check_dev(k->tab, (size_t)k->n * sizeof *k->tab, "planes range: the table")) return;
    for (t = 0; t < k->n; t++) {
        const LzPlanesRangeEntry* e = k->tab + t;
        const uint64_t E = e->elem, n8 = e->nElems - e->nElems % 8, r0 = e->first > n8 ? e->first : n8;
        const uint64_t* pp = k->pieces + e->firstPiece;
        uint8_t* dst = (uint8_t*)(uintptr_t)e->dst;
        const uint8_t* xb = (const uint8_t*)(uintptr_t)e->base;
        uint64_t i, p, b;
        if (!fh_check_dev(pp, 8 * (size_t)(e->filter ? 8 * E + 1 : E), "planes range: an item's pieces")
            || !fh_check_dev(dst, (size_t)((e->last - e->first) * E), "planes range: an item's dst")
            || (xb && !fh_check_dev(xb, (size_t)((e->last - e->first) * E), "planes range: an item's base"))) continue;
        for (i = e->first; i < e->last; i++)
            for (p = 0; p < E; p++) {
                const uint64_t at = (i - e->first) * E + p;
                uint8_t v = 0;
                if (!e->filter) v = ((const uint8_t*)(uintptr_t)pp[p])[i - e->first];
                else if (i >= n8) v = ((const uint8_t*)(uintptr_t)pp[8 * E])[(i - r0) * E + p];
                else for (b = 0; b < 8; b++) v |= (uint8_t)(((((const uint8_t*)(uintptr_t)pp[8 * p + b])[i / 8 - e->first / 8] >> (i % 8)) & 1u) << b);
                dst[at] = v ^ (xb ? xb[at] : 0);
            }
    }
}
int lzk_planes_range_launch(LzCtx* c, const LzPlanesRangeEntry* d_tab, uint32_t nEntries, const uint64_t* d_pieces, uint32_t nTiles, hipStream_t stream)
{
    RangeK k;
    (void)c;
    if (!d_tab || !d_pieces || nEntries == 0 || nTiles == 0) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_planes_range_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    g_launches[1]++;
    k.tab = d_tab; k.n = nEntries; k.pieces = d_pieces;
    return fh_enqueue_kernel(stream, range_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- one call against the full decode, range by range ---- */
void pf_shutdown(void);
#define CHECK(cond, ...) DFC_CHECK("slice_device_fake", cond, __VA_ARGS__)
#define SDF_MAX 16
#define SDF_BLOCK ((size_t)131072)
#define SDF_DATA (12 * SDF_BLOCK)
static uint8_t* g_data;
const char* sdf_last_error(void) { return dfc_text; }

/* Frame i: sizes[i] bytes at frames[i] (host memory) with ranges [firstRange[i], + nRanges[i]) of `ranges` (nr of them, lo and hi in
 * turn); the destination has `cap` bytes.  Out: results[nf], rangeAt[nr + 1], grown[4] (LizardGPU_sliceDeviceStats over the call),
 * *rcOut.  refs (may be NULL) / refSizes: where refs[i] is not NULL the full decode is made of THAT frame (the intact twin of a frame
 * damaged outside its picked blocks).  0 when the canary margins and the sources are intact, every byte of d_dst is untouched when the call returned an error,
 * and for every frame answered 0 every range holds the bytes of LizardGPU_decompressFrame_device's full decode at its place. */
int sdf_run(size_t nf, const uint8_t* const* frames, const size_t* sizes, const uint32_t* firstRange, const uint32_t* nRanges, size_t nr,
            const uint64_t* ranges, size_t cap, size_t* results, uint64_t* rangeAt, unsigned long long grown[4], int* rcOut,
            const uint8_t* const* refs, const size_t* refSizes)
{
    Region src[SDF_MAX], dst, one, twin;
    LizardGPU_sliceFrame_t fr[SDF_MAX];
    unsigned long long s0[4], s1[4];
    size_t i, g, q;
    const hipStream_t user = dfc_user();
    int rc, bad = 0;
    (void)nr;
    CHECK(nf <= SDF_MAX, "too many frames");
    for (i = 0; i < nf; i++) {
        CHECK(!region_make(&src[i], frames[i], sizes[i], i % 4, 0x5A), "allocation");
        fr[i].d_src = region_at(&src[i]); fr[i].srcSize = sizes[i]; fr[i].firstRange = firstRange[i]; fr[i].nRanges = nRanges[i];
        results[i] = 12345;
    }
    CHECK(!region_make(&dst, NULL, cap, 3, 0xC3), "allocation");
    LizardGPU_sliceDeviceStats(s0);
    rc = LizardGPU_decompressFrameRanges_device(region_at(&dst), cap, nf, fr, (const LizardGPU_byteRange_t*)ranges, rangeAt, results, user);
    dfc_keep_text();
    LizardGPU_sliceDeviceStats(s1);
    for (g = 0; g < 4; g++) grown[g] = s1[g] - s0[g];
    *rcOut = rc;
    hipStreamSynchronize(user);
    if (region_fetch(&dst)) bad = 1;
    if (!bad && rc) for (q = 0; q < cap; q++) if (region_bytes(&dst)[q] != 0xC3) { bad = 4; break; }
    for (i = 0; i < nf && !bad; i++) {
        const int other = refs && refs[i];
        size_t t, used = 0, room;
        uint32_t r;
        if (region_fetch_same(&src[i], frames[i])) { bad = 1; break; }
        if (rc || results[i]) continue;
        room = LizardGPU_decompressFrameBound(other ? refs[i] : frames[i], other ? refSizes[i] : sizes[i]);
        CHECK(!LizardGPU_frameIsError(room), "the bound of a frame the entry answered");
        CHECK(!region_make(&one, NULL, room, 1, 0xC3) && (!other || !region_make(&twin, refs[i], refSizes[i], 2, 0x5A)), "allocation");
        t = LizardGPU_decompressFrame_device(region_at(&one), room, other ? region_at(&twin) : fr[i].d_src, other ? refSizes[i] : sizes[i], &used,
                                             LIZARDGPU_FRAME_SKIP_CHECKSUM, user);
        hipStreamSynchronize(user);
        if (region_fetch(&one)) bad = 5;
        if (other) region_free(&twin);
        if (!bad && LizardGPU_frameIsError(t)) bad = 2;
        for (r = 0; r < nRanges[i] && !bad; r++) {
            const uint64_t lo = ranges[2 * (firstRange[i] + r)], hi = ranges[2 * (firstRange[i] + r) + 1];
            const uint64_t at = rangeAt[firstRange[i] + r] + lo % SDF_BLOCK;
            if (hi <= lo) { if (rangeAt[firstRange[i] + r + 1] != rangeAt[firstRange[i] + r]) bad = 6; continue; }
            if (hi > t || at + (hi - lo) > cap) bad = 3;
            else if (memcmp(region_bytes(&dst) + at, region_bytes(&one) + lo, (size_t)(hi - lo))) bad = 3;
        }
        region_free(&one);
        if (bad) fprintf(stderr, "slice_device_fake: frame %zu of %zu: %s (call returned %d): %s\n", i, nf,
                         bad == 2 ? "the single entry refuses a frame the slice entry answered" : bad == 3 ? "a range's bytes differ from the full decode's"
                         : bad == 6 ? "an empty range takes room" : "the single entry wrote outside its d_dst", rc, dfc_text);
    }
    if (bad == 1) fprintf(stderr, "slice_device_fake: a canary margin or a source changed\n");
    if (bad == 4) fprintf(stderr, "slice_device_fake: a failed call wrote into d_dst\n");
    for (i = 0; i < nf; i++) region_free(&src[i]);
    region_free(&dst);
    CHECK(!bad, "the call is wrong");
    return 0;
}

/* ---- the frames of the tests ---- */
static const uint8_t* sdf_data(void)
{
    if (!g_data) {
        unsigned long long x = 0x9E3779B97F4A7C15ull;
        size_t i;
        g_data = (uint8_t*)malloc(SDF_DATA);
        lzo_datagen(g_data, SDF_DATA, 0.5, 0.0, 77u);
        for (i = 2 * SDF_BLOCK - 5000; i < 3 * SDF_BLOCK + 4000; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; g_data[i] = (uint8_t)(x >> 32); }      /* raw records between compressed ones */
    }
    return g_data;
}

/* n bytes of the test data from `off` as one frame of 128 KiB independent blocks; the frame's bytes, or a frame error code */
size_t sdf_frame(uint8_t* out, size_t cap, size_t off, size_t n, int level, int checksum, int csize)
{
    LizardF_preferences_t p;
    if (off + n > SDF_DATA) return LZ_FRAME_E(GENERIC);
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)1; p.frameInfo.blockMode = (LizardF_blockMode_t)1;
    p.frameInfo.contentChecksumFlag = (LizardF_contentChecksum_t)checksum; p.frameInfo.contentSize = csize ? n : 0; p.compressionLevel = level;
    return LizardGPU_compressFrame(out, cap, sdf_data() + off, n, &p);
}

/* a FLUSHED frame with its content size: `head` bytes (a short record), a flush, then n - head bytes: the record count is
 * ceil(n / 128 KiB) when head is under a block and n - head is a whole number of blocks, but record 0 does not fill its block */
size_t sdf_flushed_frame(uint8_t* out, size_t cap, size_t off, size_t head, size_t n, int level)
{
    LizardF_compressionContext_t cctx;
    LizardF_preferences_t p;
    size_t at = 0, r;
    if (off + n > SDF_DATA || head > n) return LZ_FRAME_E(GENERIC);
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)1; p.frameInfo.blockMode = (LizardF_blockMode_t)1; p.frameInfo.contentSize = n; p.compressionLevel = level;
    if (LizardF_isError(LizardF_createCompressionContext(&cctx, 100))) return LZ_FRAME_E(GENERIC);
#define STEP(call) do { r = (call); if (LizardF_isError(r)) { LizardF_freeCompressionContext(cctx); return r; } at += r; } while (0)
    STEP(LizardF_compressBegin(cctx, out + at, cap - at, &p));
    STEP(LizardF_compressUpdate(cctx, out + at, cap - at, sdf_data() + off, head, NULL));
    STEP(LizardF_flush(cctx, out + at, cap - at, NULL));
    STEP(LizardF_compressUpdate(cctx, out + at, cap - at, sdf_data() + off + head, n - head, NULL));
    STEP(LizardF_compressEnd(cctx, out + at, cap - at, NULL));
#undef STEP
    LizardF_freeCompressionContext(cctx);
    return at;
}

/* LizardGPU_joinPlanesRange_device on the fake: `split` (size bytes: the split content of n elements of E bytes) goes up, every range
 * of LizardGPU_planesRangeBytes becomes a piece INSIDE it, elements [first, last) are joined into `out` ((last - first) * E bytes),
 * XORed with `base` (may be NULL: none).  The call's return value, or 1000 for a failure of the harness. */
int sdf_join(const uint8_t* split, size_t size, uint64_t n, uint32_t E, uint32_t filter, uint64_t first, uint64_t last, const uint8_t* base, uint8_t* out)
{
    LizardGPU_byteRange_t ranges[R_MAX_PIECES];
    const void* pieces[R_MAX_PIECES];
    LizardGPU_planesRange_t item;
    Region src, dst, xb;
    const size_t bytes = (size_t)((last - first) * E), nr = LizardGPU_planesRangeBytes(n, E, filter, first, last, ranges, R_MAX_PIECES);
    const hipStream_t user = dfc_user();
    size_t q;
    int rc;
    if (!nr || region_make(&src, split, size, 1, 0x5A) || region_make(&dst, NULL, bytes, 2, 0xC3) || region_make(&xb, base, base ? bytes : 0, 3, 0x77)) return 1000;
    for (q = 0; q < nr; q++) pieces[q] = region_at(&src) + ranges[q].lo;
    memset(&item, 0, sizeof item);
    item.d_dst = region_at(&dst); item.d_base = base ? region_at(&xb) : NULL; item.nElems = n; item.first = first; item.last = last;
    item.elemSize = E; item.filter = filter; item.firstPiece = 0;
    rc = LizardGPU_joinPlanesRange_device(1, &item, pieces, user);
    hipStreamSynchronize(user);
    if (region_fetch(&dst) || region_fetch(&src) || region_fetch(&xb)) rc = 1000;
    else memcpy(out, region_bytes(&dst), bytes);
    region_free(&src); region_free(&dst); region_free(&xb);
    return rc;
}

#ifdef SLICE_DEVICE_FAKE_MAIN
/* ---- the program form, for the sanitizer build: a batch of good frames and one of refused ones, under four schedules ---- */
void fh_set_schedule(int mode, unsigned seed);
int main(void)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 }, { FH_RANDOM, 12 } };
    static const uint8_t skippable[] = { 0x57, 0x2A, 0x4D, 0x18, 5, 0, 0, 0, 's', 'k', 'i', 'p', '!' };
    const size_t bs = SDF_BLOCK, slot = 4 * SDF_BLOCK;
    uint8_t* pool = (uint8_t*)malloc(8 * slot);
    size_t s;
    CHECK(pool, "allocation");
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++) {
        const int level = s & 2 ? 30 : 10;
        const uint8_t* frames[8]; size_t sizes[8], results[8], n = 0, f;
        /* per frame two ranges: inside one block / across a block edge, ending at C / empty, two in one block */
        const uint32_t firstRange[8] = { 0, 2, 4, 6, 8, 10, 12, 14 }, nRanges[8] = { 2, 2, 2, 2, 2, 2, 2, 2 };
        const uint64_t ranges[32] = { 100, 2000, bs - 10, bs + 10,   2 * bs + 5, 3 * bs, 7, 7,   10, 20, 30, 40,   0, 0, 0, 0,
                                      0, 10, 0, 0,   0, 1, 0, 0,   0, 10, 0, 0,   0, 3 * bs + 1, 0, 0 };
        uint64_t rangeAt[17];
        unsigned long long grown[4], before;
        int rc;
        fh_set_schedule(sched[s].mode, sched[s].seed);
        if (s == 1) pf_shutdown();
#define ADD(bytes) do { frames[n] = pool + n * slot; sizes[n] = (bytes); n++; } while (0)
        f = sdf_frame(pool + n * slot, slot, 0, 3 * bs, level, (int)(s & 1), 1); CHECK(!LizardF_isError(f), "frame"); ADD(f);
        f = sdf_frame(pool + n * slot, slot, 0, 3 * bs, level, 0, 1); CHECK(!LizardF_isError(f), "frame"); ADD(f);
        f = sdf_frame(pool + n * slot, slot, 5 * bs, bs - 100, level, 1, 1); CHECK(!LizardF_isError(f), "frame"); ADD(f);
        f = sdf_frame(pool + n * slot, slot, 0, 0, level, 0, 0); CHECK(!LizardF_isError(f), "frame"); ADD(f);                 /* no blocks: empty ranges only */
        f = sdf_frame(pool + n * slot, slot, 0, bs, level, 0, 0); CHECK(!LizardF_isError(f), "frame"); ADD(f);                /* refused: no content size */
        memcpy(pool + n * slot, skippable, sizeof skippable); ADD(sizeof skippable);                                           /* refused: skippable */
        f = sdf_frame(pool + n * slot, slot, 0, 2 * bs, level, 0, 1); CHECK(!LizardF_isError(f), "frame"); ADD(f / 2);        /* refused: cut in its chain */
        f = sdf_frame(pool + n * slot, slot, 0, 3 * bs, level, 0, 1); CHECK(!LizardF_isError(f), "frame"); ADD(f);            /* refused: hi > C */
#undef ADD
        CHECK(!sdf_run(n, frames, sizes, firstRange, nRanges, 16, ranges, 6 * bs, results, rangeAt, grown, &rc, NULL, NULL), "the batch");
        CHECK(rc == 0 && !results[0] && !results[1] && !results[2] && !results[3], "the good frames: %d %zu %zu %zu %zu: %s", rc, results[0], results[1], results[2], results[3], dfc_text);
        CHECK(results[4] == LZ_FRAME_E(frameSize_wrong) && results[5] == LZ_FRAME_E(frameType_unknown) && LizardGPU_frameIsError(results[6]) && results[7] == LZ_FRAME_E(frameSize_wrong), "the refusals");
        CHECK(rangeAt[16] == 6 * bs && grown[0] == 6 && grown[1] == 4 && grown[2] == 4 && grown[3] == 1, "places and statistics: %llu bytes, %llu %llu %llu %llu",
              (unsigned long long)rangeAt[16], grown[0], grown[1], grown[2], grown[3]);
        before = sdf_launches(0);
        CHECK(!sdf_run(n, frames, sizes, firstRange, nRanges, 16, ranges, 6 * bs - 1, results, rangeAt, grown, &rc, NULL, NULL), "one byte short");
        CHECK(rc == -LIZARDGPU_ERR_ARG && strstr(dfc_text, "dstMaxSize_tooSmall") && sdf_launches(0) == before, "one byte short: %d, %s", rc, dfc_text);
    }
    free(pool);
    printf("slice_device_fake: ok, %llu ops\n", fh_ops_run());
    return 0;
}
#endif
