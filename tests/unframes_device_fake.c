/* tests/unframes_device_fake.c — TEST INFRASTRUCTURE: lizard_amd/csrc/lizard_unframes_device.c (LizardGPU_decompressFrames_device /
 * LizardGPU_framesInfo_device: a count pass and a fill pass over a batch of frames, two host waits, everything behind the first wait
 * enqueued at once on one stream, the frames that are not clean handed to the single-frame entry) compiled as a unit under test on a
 * CPU, on the fake HIP runtime with DEFERRED streams.  Linked with tests/pipeline_fake.c (the context, the single-frame entry
 * LizardGPU_decompressFrame_device and the host twins on the same fake, the emulator's record decoder and walk) and tests/fake_hip.c as
 * they are; this file adds the shims they do not have: plain sequential models of lz_unframes_walk_kernel (the real walk on the
 * emulator, frame after frame), lz_unframes_kernel (the emulator's record decoder, records in a shuffled order),
 * lz_unframes_settle_kernel, lz_xxh32_frames_kernel and lz_unframes_finish_kernel that check that everything they touch lies in live
 * device memory.
 * udf_refuse(kind, nth): the n-th launch of that kind from now answers -LIZARDGPU_ERR_HIP, once, and enqueues nothing.
 * udf_batch runs one batch of caller-given frames and compares every frame with LizardGPU_decompressFrame_device on the same fake;
 * udf_cases builds the standard batch of the tests and runs it.  Both forms have them.
 *   library : with pipeline_fake.c, -shared (tests/test_frames_decompress_fake_device.py drives it through ctypes)
 *   program : -DUNFRAMES_DEVICE_FAKE_MAIN, for the sanitizer build: argv[1] = tests/golden/frame_ref_linked.liz; exit 0 = all good */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../lizard_amd/csrc/lizard_unframes_device.c"     /* unit under test, compiled into this harness */
#include "device_fake_common.h"
#include "lizard_oracle.h"

unsigned emul_unframe_record(const void* payload, unsigned size, unsigned word, void* slot, unsigned cap, unsigned seed);      /* tests/pipeline_fake_emul.cpp */
void emul_walk_segment(const void* src, unsigned long long srcSize, unsigned long long startPos, unsigned long long budget,
                       unsigned long long tableCap, unsigned long long* offs, unsigned* words, void* res, unsigned seed);

enum { UDF_WALK, UDF_DECODE, UDF_SETTLE, UDF_FINISH, UDF_KINDS };
void udf_refuse(int kind, int nth) { if (kind < UDF_KINDS) dfc_refuse_set(kind, nth); }

/* ---- lz_unframes_walk_kernel ---- */
typedef struct { const LzUnframesEntry* frames; uint32_t n, want; uint64_t* offs; uint32_t* words; LzWalkResult* res; } WalkK;
static void walk_kernel(void* a)
{
    const WalkK* k = (const WalkK*)a;
    uint32_t f;
    if (!fh_check_dev(k->frames, (size_t)k->n * sizeof *k->frames, "unframes walk: the frame table")
        || !fh_check_dev(k->res, (size_t)k->n * sizeof *k->res, "unframes walk: the result records")) return;
    for (f = 0; f < k->n; f++) {
        const LzUnframesEntry* e = k->frames + f;
        if (!(e->flags & k->want)) continue;
        if (e->srcSize && !fh_check_dev((const void*)(uintptr_t)e->src, (size_t)e->srcSize, "unframes walk: a frame's src[0..srcSize)")) continue;
        if (k->offs && e->nRecords && (!fh_check_dev(k->offs + e->first, 8 * (size_t)e->nRecords, "unframes walk: a frame's region of the offset table")
                                       || !fh_check_dev(k->words + e->first, 4 * (size_t)e->nRecords, "unframes walk: a frame's region of the word table"))) continue;
        emul_walk_segment((const void*)(uintptr_t)e->src, e->srcSize, 0, ~0ull, e->nRecords, k->offs ? (unsigned long long*)(k->offs + e->first) : NULL,
                          k->words ? k->words + e->first : NULL, k->res + f, fh_rand() | 1u);
    }
}
int lzk_unframes_walk_launch(const LzUnframesEntry* d_frames, uint32_t nFrames, int fill, uint64_t* d_offs, uint32_t* d_words, LzWalkResult* d_res,
                             hipStream_t stream)
{
    WalkK k;
    if (!d_frames || !d_res || nFrames == 0 || (fill && (!d_offs || !d_words))) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_unframes_walk_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    if (dfc_refused(UDF_WALK, "lzk_unframes_walk_launch")) return -LIZARDGPU_ERR_HIP;
    k.frames = d_frames; k.n = nFrames; k.want = fill ? LZU_DECODE : LZU_WALK; k.offs = fill ? d_offs : NULL; k.words = fill ? d_words : NULL; k.res = d_res;
    return fh_enqueue_kernel(stream, walk_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- lz_unframes_kernel: one wave per record, in whatever order the waves claim them ---- */
typedef struct { const LzUnframesEntry* frames; const uint64_t* offs; const uint32_t *words, *recFrame; uint32_t* out; size_t n; } DecodeK;
static void decode_kernel(void* a)
{
    const DecodeK* k = (const DecodeK*)a;
    uint32_t* order = (uint32_t*)malloc(k->n * sizeof *order);
    size_t i;
    if (!fh_check_dev(k->offs, 8 * k->n, "unframes decode: payload offsets") || !fh_check_dev(k->words, 4 * k->n, "unframes decode: words")
        || !fh_check_dev(k->recFrame, 4 * k->n, "unframes decode: the records' frames") || !fh_check_dev(k->out, 4 * k->n, "unframes decode: results")) { free(order); return; }
    dfc_shuffled(order, k->n);
    for (i = 0; i < k->n; i++) {
        const uint32_t b = order[i], word = k->words[b], size = word & 0x7FFFFFFFu;
        const LzUnframesEntry* e = k->frames + k->recFrame[b];
        uint64_t at, room;
        uint32_t r = 0xFFFFFFFFu;
        if (!fh_check_dev(e, sizeof *e, "unframes decode: a record's frame entry")) continue;
        at = ((uint64_t)b - e->first) * e->maxBlock;
        if (at < e->cap) {
            room = e->cap - at < e->maxBlock ? e->cap - at : e->maxBlock;
            if (!fh_check_dev((uint8_t*)(uintptr_t)e->dst + at, (size_t)room, "unframes decode: a record's slot in its d_dst")) continue;
            if (size && size <= room && !fh_check_dev((const uint8_t*)(uintptr_t)e->src + k->offs[b], size, "unframes decode: a record's payload")) continue;
            r = emul_unframe_record((const uint8_t*)(uintptr_t)e->src + k->offs[b], size, word, (uint8_t*)(uintptr_t)e->dst + at, (uint32_t)room, fh_rand() | 1u);
        }
        k->out[b] = r;
    }
    free(order);
}
int lzk_unframes_decode_launch(LzCtx* c, const LzUnframesEntry* d_frames, const uint64_t* d_offs, const uint32_t* d_words, const uint32_t* d_recFrame,
                               uint32_t* d_out, size_t nRecords, hipStream_t stream)
{
    DecodeK k;
    if (!d_frames || !d_offs || !d_words || !d_recFrame || !d_out || nRecords == 0 || nRecords > 0xFFFFFFFFu) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_unframes_decode_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    if (dfc_refused(UDF_DECODE, "lzk_unframes_decode_launch")) return -LIZARDGPU_ERR_HIP;
    k.frames = d_frames; k.offs = d_offs; k.words = d_words; k.recFrame = d_recFrame; k.out = d_out; k.n = nRecords;
    c->hostKernelMs = -1.0f;
    return fh_enqueue_kernel(stream, decode_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- lz_unframes_settle_kernel ---- */
typedef struct { const LzUnframesEntry* frames; uint32_t n; const uint32_t* out; LzUnframesResult* results; LzFramesEntry* hash; } SettleK;
static void settle_kernel(void* a)
{
    const SettleK* k = (const SettleK*)a;
    uint32_t f, i;
    if (!fh_check_dev(k->frames, (size_t)k->n * sizeof *k->frames, "unframes settle: the frame table")
        || !fh_check_dev(k->results, (size_t)k->n * sizeof *k->results, "unframes settle: the result records")
        || !fh_check_dev(k->hash, (size_t)k->n * sizeof *k->hash, "unframes settle: the hash table")) return;
    for (f = 0; f < k->n; f++) {
        const LzUnframesEntry* e = k->frames + f;
        LzUnframesResult r = { 0, LZU_DEAD, 0 };
        if (e->flags & LZU_DECODE) {
            int clean = 1;
            if (e->nRecords && !fh_check_dev(k->out + e->first, 4 * (size_t)e->nRecords, "unframes settle: a frame's per-record results")) continue;
            for (i = 0; i < e->nRecords; i++) {
                const uint32_t v = k->out[e->first + i];
                if (v >= LZU_NEED_HISTORY || (i + 1 < e->nRecords && v != e->maxBlock)) clean = 0;
                else r.size += v;
            }
            r.state = clean ? LZU_CLEAN : LZU_DELEGATE;
            if (!clean) r.size = 0;
        }
        k->results[f] = r;
        k->hash[f].srcSize = r.size;
    }
}
int lzk_unframes_settle_launch(const LzUnframesEntry* d_frames, uint32_t nFrames, const uint32_t* d_out, LzUnframesResult* d_results, LzFramesEntry* d_hashTab,
                               hipStream_t stream)
{
    SettleK k;
    if (!d_frames || !d_out || !d_results || !d_hashTab || nFrames == 0) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_unframes_settle_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    if (dfc_refused(UDF_SETTLE, "lzk_unframes_settle_launch")) return -LIZARDGPU_ERR_HIP;
    k.frames = d_frames; k.n = nFrames; k.out = d_out; k.results = d_results; k.hash = d_hashTab;
    return fh_enqueue_kernel(stream, settle_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- lz_xxh32_frames_kernel, over the decoded frames ---- */
int lzk_frames_hash_launch(LzFramesEntry* d_frames, uint32_t nFrames, hipStream_t stream) { return dfc_frames_hash_launch(d_frames, nFrames, stream); }

/* ---- lz_unframes_finish_kernel ---- */
typedef struct { const LzUnframesEntry* frames; uint32_t n; const LzFramesEntry* hash; LzUnframesResult* results; } FinishK;
static void finish_kernel(void* a)
{
    const FinishK* k = (const FinishK*)a;
    uint32_t f;
    if (!fh_check_dev(k->frames, (size_t)k->n * sizeof *k->frames, "unframes finish: the frame table")
        || !fh_check_dev(k->results, (size_t)k->n * sizeof *k->results, "unframes finish: the result records")
        || !fh_check_dev(k->hash, (size_t)k->n * sizeof *k->hash, "unframes finish: the hash table")) return;
    for (f = 0; f < k->n; f++) {
        const LzUnframesEntry* e = k->frames + f;
        LzUnframesResult* r = k->results + f;
        if (r->state != LZU_CLEAN) continue;
        if (e->contentSize && r->size != e->contentSize) r->state = LZU_DELEGATE;
        else if (e->flags & LZU_VERIFY) {
            const uint8_t* p = (const uint8_t*)(uintptr_t)e->src + e->frameBytes - 4;
            if (e->frameBytes < 4 || e->frameBytes > e->srcSize || !fh_check_dev(p, 4, "unframes finish: a frame's stored checksum")) continue;
            if (((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)) != k->hash[f].hash) r->state = LZU_DELEGATE;
        }
        if (r->state != LZU_CLEAN) r->size = 0;
    }
}
int lzk_unframes_finish_launch(const LzUnframesEntry* d_frames, uint32_t nFrames, const LzFramesEntry* d_hashTab, LzUnframesResult* d_results, hipStream_t stream)
{
    FinishK k;
    if (!d_frames || !d_hashTab || !d_results || nFrames == 0) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_unframes_finish_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    if (dfc_refused(UDF_FINISH, "lzk_unframes_finish_launch")) return -LIZARDGPU_ERR_HIP;
    k.frames = d_frames; k.n = nFrames; k.hash = d_hashTab; k.results = d_results;
    return fh_enqueue_kernel(stream, finish_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- one batch against the single-frame entry, frame by frame ---- */
void pf_shutdown(void);
#define CHECK(cond, ...) DFC_CHECK("unframes_device_fake", cond, __VA_ARGS__)
#define UDF_MAX 16
#define UDF_BLOCK ((size_t)131072)
#define UDF_DATA (12 * UDF_BLOCK)
static uint8_t* g_data;
const char* udf_last_error(void) { return dfc_text; }            /* LizardGPU_lastError as the last batch left it (the single entry's calls come behind it) */

/* Frame i: sizes[i] bytes at frames[i] (host memory), capacity caps[i]; nullIdx >= 0: that entry's destination is NULL.  wantRc: what
 * the call must return.  0: every results[i], consumed[i] and the decoded bytes equal LizardGPU_decompressFrame_device's for the same
 * bytes and capacity on the same fake.  Else: every frame answers GENERIC with 0 consumed, or what the single entry answers when the
 * count pass had decided it.  failMalloc: the n-th hipMalloc inside the call fails.  grown (may be NULL): the growth of
 * LizardGPU_framesDecodeDeviceStats over the call. */
int udf_batch(size_t nf, const uint8_t* const* frames, const size_t* sizes, const size_t* caps, unsigned flags, int nullIdx, int failMalloc, int wantRc,
              unsigned long long grown[4])
{
    Region src[UDF_MAX], dst[UDF_MAX], one;
    void* dsts[UDF_MAX]; const void* srcs[UDF_MAX];
    size_t results[UDF_MAX], used[UDF_MAX], i, g;
    unsigned long long s0[4], s1[4];
    const hipStream_t user = dfc_user();
    int rc, bad = 0;
    CHECK(nf <= UDF_MAX, "too many frames");
    for (i = 0; i < nf; i++) {
        CHECK(!region_make(&src[i], frames[i], sizes[i], i % 4, 0x5A) && !region_make(&dst[i], NULL, caps[i], (3 * i) % 4, 0xC3), "allocation");
        srcs[i] = region_at(&src[i]); dsts[i] = (int)i == nullIdx ? NULL : region_at(&dst[i]); results[i] = 12345; used[i] = 12345;
    }
    if (failMalloc) hipStreamSynchronize(user);          /* (a call that fails before it orders itself behind the caller's stream leaves that stream's work queued, as it may) */
    LizardGPU_framesDecodeDeviceStats(s0);
    fh_fail_malloc(failMalloc);
    rc = LizardGPU_decompressFrames_device(nf, dsts, caps, srcs, sizes, results, used, flags, user);
    fh_fail_malloc(0);
    dfc_keep_text();
    LizardGPU_framesDecodeDeviceStats(s1);
    for (g = 0; g < 4 && grown; g++) grown[g] = s1[g] - s0[g];
    hipStreamSynchronize(user);                          /* (a call that decided every frame up front never touched the caller's stream) */
    for (i = 0; i < nf && !bad; i++) {
        size_t t, tUsed = 777;
        if (region_fetch_same(&src[i], frames[i]) || region_fetch(&dst[i])) { bad = 1; break; }
        if (wantRc && results[i] == LZ_FRAME_E(GENERIC) && !used[i]) continue;      /* (a frame the failed call had not decided: nothing to compare) */
        CHECK(!region_make(&one, NULL, caps[i], (3 * i) % 4, 0xC3), "allocation");
        t = LizardGPU_decompressFrame_device((int)i == nullIdx ? NULL : region_at(&one), caps[i], srcs[i], sizes[i], &tUsed, flags, user);
        hipStreamSynchronize(user);                      /* (a call that refuses its arguments never touched the caller's stream) */
        if (region_fetch(&one)) bad = 5;
        if (!bad && wantRc && !(results[i] == LZ_FRAME_E(GENERIC) || (LizardGPU_frameIsError(t) && results[i] == t) || (!t && !results[i] && used[i] == tUsed))) bad = 2;
        if (!bad && wantRc && results[i] == LZ_FRAME_E(GENERIC) && used[i]) bad = 2;
        if (!bad && !wantRc && (results[i] != t || used[i] != tUsed)) bad = 2;
        if (!bad && !wantRc && !LizardGPU_frameIsError(t) && t && memcmp(region_bytes(&dst[i]), region_bytes(&one), t)) bad = 3;
        region_free(&one);
        if (bad) fprintf(stderr, "unframes_device_fake: frame %zu of %zu: %s (result %zu consumed %zu, single entry %zu consumed %zu; %zu bytes, cap %zu, flags %u; call returned %d): %s\n",
                         i, nf, bad == 2 ? "unexpected result" : bad == 3 ? "decoded bytes differ from the single entry's" : "the single entry wrote outside its d_dst",
                         results[i], used[i], t, tUsed, sizes[i], caps[i], flags, rc, dfc_text);
    }
    if (bad == 1) fprintf(stderr, "unframes_device_fake: frame %zu of %zu: a canary margin or the source changed\n", i, nf);
    for (i = 0; i < nf; i++) { region_free(&src[i]); region_free(&dst[i]); }
    CHECK(!bad, "a frame of the batch is wrong");
    CHECK(rc == wantRc, "the call returned %d, wanted %d: %s", rc, wantRc, dfc_text);
    return 0;
}

/* ---- the standard batch ---- */
static const uint8_t* udf_data(void)
{
    if (!g_data) {
        unsigned long long x = 0x9E3779B97F4A7C15ull;
        size_t i;
        g_data = (uint8_t*)malloc(UDF_DATA);
        lzo_datagen(g_data, UDF_DATA, 0.5, 0.0, 77u);
        for (i = 2 * UDF_BLOCK - 5000; i < 3 * UDF_BLOCK + 4000; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; g_data[i] = (uint8_t)(x >> 32); }      /* raw records between compressed ones */
    }
    return g_data;
}

static size_t make_frame(uint8_t* out, size_t cap, size_t off, size_t n, int level, int checksum, int csize)
{
    LizardF_preferences_t p;
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)1; p.frameInfo.blockMode = (LizardF_blockMode_t)1;
    p.frameInfo.contentChecksumFlag = (LizardF_contentChecksum_t)checksum; p.frameInfo.contentSize = csize ? n : 0; p.compressionLevel = level;
    return LizardGPU_compressFrame(out, cap, udf_data() + off, n, &p);
}

#define UDF_SLOT (6 * UDF_BLOCK)
/* Twelve frames, 14 block records in the batch part: clean frames of 3, 1 and 0 blocks and a byte; 2 blocks one byte short of capacity; a
 * flushed frame (a short record in the middle: two frames of this library spliced); the reference's linked frame (golden, its path
 * in goldenPath, or left out when NULL); a frame cut in its header and one cut in its chain; a frame with a corrupt block; a frame with
 * a wrong checksum (when checksum is on); a skippable frame.  nullIdx as in udf_batch. */
int udf_cases(int level, int checksum, int csize, unsigned flags, const char* goldenPath, int nullIdx, int failMalloc, int wantRc, unsigned long long grown[4])
{
    static uint8_t* pool;
    static const uint8_t skippable[] = { 0x57, 0x2A, 0x4D, 0x18, 5, 0, 0, 0, 's', 'k', 'i', 'p', '!', 't', 'a', 'i', 'l' };
    const size_t bs = UDF_BLOCK;
    const uint8_t* frames[UDF_MAX]; size_t sizes[UDF_MAX], caps[UDF_MAX], n = 0, f, a, b;
    uint8_t* at;
    if (!pool) pool = (uint8_t*)malloc(UDF_MAX * UDF_SLOT);
    at = pool;
#define ADD(bytes, cap_) do { frames[n] = at; sizes[n] = (bytes); caps[n] = (cap_); at += UDF_SLOT; n++; } while (0)
    f = make_frame(at, UDF_SLOT, 0, 3 * bs, level, checksum, csize); CHECK(!LizardF_isError(f), "frame"); ADD(f, 3 * bs);           /* 0: raw and compressed records */
    f = make_frame(at, UDF_SLOT, 3 * bs, bs, level, checksum, csize); CHECK(!LizardF_isError(f), "frame"); ADD(f, bs + 100);
    f = make_frame(at, UDF_SLOT, 0, 0, level, checksum, 0); CHECK(!LizardF_isError(f), "frame"); ADD(f, 0);
    f = make_frame(at, UDF_SLOT, 4 * bs, 2 * bs, level, checksum, csize); CHECK(!LizardF_isError(f), "frame"); ADD(f, 2 * bs - 1);   /* 3: one byte short */
    a = make_frame(at, UDF_SLOT, 6 * bs, 70000, level, 0, 0); CHECK(!LizardF_isError(a), "frame");                                   /* 4: flushed: a short record, then a full one */
    b = make_frame(at + a - 4, UDF_SLOT - a, 7 * bs, bs, level, 0, 0); CHECK(!LizardF_isError(b), "frame");
    memmove(at + a - 4, at + a - 4 + 7, b - 7); ADD(a - 4 + b - 7, 70000 + bs);
    if (goldenPath) {                                                                                                                /* 5: linked, needs its history */
        FILE* fp = fopen(goldenPath, "rb");
        CHECK(fp, "cannot open %s", goldenPath);
        f = fread(at, 1, UDF_SLOT, fp); fclose(fp);
        CHECK(f > 15 && f < UDF_SLOT, "golden frame"); ADD(f, LizardGPU_decompressFrameBound(at, f));
    }
    f = make_frame(at, UDF_SLOT, 8 * bs, bs, level, checksum, 1); CHECK(!LizardF_isError(f), "frame"); ADD(9, bs);                  /* cut in its header */
    f = make_frame(at, UDF_SLOT, 8 * bs, 2 * bs, level, checksum, csize); CHECK(!LizardF_isError(f), "frame"); ADD(f / 2, 2 * bs);   /* cut in its chain */
    f = make_frame(at, UDF_SLOT, 9 * bs, bs, level, checksum, csize); CHECK(!LizardF_isError(f), "frame");                           /* a corrupt block */
    memset(at + (csize ? 15 : 7) + 4 + 3, 0xFF, 40); ADD(f, bs);
    f = make_frame(at, UDF_SLOT, 10 * bs, bs, level, checksum, csize); CHECK(!LizardF_isError(f), "frame");                          /* a wrong checksum */
    if (checksum) at[f - 2] ^= 0x10;
    ADD(f, bs);
    memcpy(at, skippable, sizeof skippable); ADD(sizeof skippable, 10);
    f = make_frame(at, UDF_SLOT, 777, 1, level, checksum, 0); CHECK(!LizardF_isError(f), "frame"); ADD(f, 1);
#undef ADD
    return udf_batch(n, frames, sizes, caps, flags, nullIdx, failMalloc, wantRc, grown);
}

#ifdef UNFRAMES_DEVICE_FAKE_MAIN
/* ---- the program form, for the sanitizer build: the standard batch over schedules, levels, checksum, flags, refusals and failures ---- */
void fh_set_schedule(int mode, unsigned seed);
int main(int argc, char** argv)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 }, { FH_RANDOM, 12 } };
    const char* golden = argc > 1 ? argv[1] : NULL;
    unsigned long long grown[4];
    size_t s;
    int kind;
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++) {
        const int checksum = (int)(s & 1) ^ 1, level = s & 2 ? 30 : 10;
        fh_set_schedule(sched[s].mode, sched[s].seed);
        if (s == 1) pf_shutdown();
        if (udf_cases(level, checksum, (int)(s & 1), 0, golden, -1, 0, 0, grown)) return 1;
        CHECK(grown[3] == 1 && grown[2] >= 5 && grown[1] >= 3 && grown[1] + grown[2] == 9, "statistics: %llu records, %llu settled, %llu delegated, %llu calls", grown[0], grown[1], grown[2], grown[3]);
        if (udf_cases(level, 1, 0, LIZARDGPU_FRAME_SKIP_CHECKSUM, NULL, 1, 0, 0, NULL)) return 1;
        for (kind = 0; kind < UDF_KINDS; kind++) {
            udf_refuse(kind, kind == UDF_WALK ? 1 + (int)(s & 1) : 1);
            if (udf_cases(level, checksum, 0, 0, NULL, -1, 0, -LIZARDGPU_ERR_HIP, NULL)) return 1;
        }
        pf_shutdown();
        if (udf_cases(level, checksum, 0, 0, NULL, -1, 1 + (int)(s % 2), -LIZARDGPU_ERR_NOMEM, NULL)) return 1;
        if (udf_cases(level, checksum, 0, 0, NULL, -1, 0, 0, NULL)) return 1;
    }
    printf("unframes_device_fake: ok, %llu ops\n", fh_ops_run());
    return 0;
}
#endif
