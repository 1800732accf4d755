/* tests/frames_device_fake.c — TEST INFRASTRUCTURE: lizard_amd/csrc/lizard_frames_device.c (LizardGPU_compressFrames_device: the blocks of
 * many frames as one list of chunks enqueued up front on three streams, the stages' slots rotating under events, one cursor per frame
 * carried in device memory, the checksums and the frames' heads and tails written by kernels) compiled as a unit under test on a CPU,
 * on the fake HIP runtime with DEFERRED streams.  Linked with tests/pipeline_fake.c (the context, lzk_launch = the oracle as the block
 * kernels over a ragged batch, the host twin LizardGPU_compressFrame on the same fake) and tests/fake_hip.c as they are; this file adds
 * the shims they do not have: plain sequential models of lz_frames_scan_kernel + lz_frames_gather_kernel, lz_xxh32_frames_kernel and
 * lz_frames_finish_kernel (lz_frames_pack.h) that check that everything they touch lies in live device memory.
 * pf_refuse_frames_pack: the n-th pack launch from now answers -LIZARDGPU_ERR_HIP, once, and enqueues nothing.
 * fdf_batch runs one batch and compares every frame with LizardGPU_compressFrame on the same bytes; both forms have it.
 *   library : with pipeline_fake.c, -shared (tests/test_frames_compress_fake_device.py drives it through ctypes)
 *   program : -DFRAMES_DEVICE_FAKE_MAIN, for the sanitizer build: exit 0 = all good */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../lizard_amd/csrc/lizard_frames_device.c"       /* unit under test, compiled into this harness */
#include "device_fake_common.h"
#include "lizard_oracle.h"

void pf_refuse_frames_pack(int nth) { dfc_refuse_set(0, nth); }

/* ---- lz_frames_scan_kernel + lz_frames_gather_kernel: block after block, each frame's cursor advancing as its records are placed ---- */
typedef struct { const uint8_t* base; const uint64_t* blkOffsets; const uint32_t *blkSizes, *blkFrames; const uint8_t* slots; size_t slot;
                 const uint32_t* sizes; uint64_t* offsets; uint32_t nb; LzFramesEntry* frames; } FramesPackK;
static void frames_pack_kernel(void* a)
{
    const FramesPackK* k = (const FramesPackK*)a;
    uint32_t b;
    if (!fh_check_dev(k->sizes, 4 * (size_t)k->nb, "frames pack: sizes") || !fh_check_dev(k->offsets, 8 * (size_t)k->nb, "frames pack: offsets")
        || !fh_check_dev(k->blkOffsets, 8 * (size_t)k->nb, "frames pack: block offsets") || !fh_check_dev(k->blkSizes, 4 * (size_t)k->nb, "frames pack: block sizes")
        || !fh_check_dev(k->blkFrames, 4 * (size_t)k->nb, "frames pack: block frames")) return;
    for (b = 0; b < k->nb; b++) {
        LzFramesEntry* e = k->frames + k->blkFrames[b];
        const uint32_t n = k->blkSizes[b], cs = k->sizes[b];
        const int isRaw = n != 1u && (cs == 0u || cs > n - 1u);
        const uint32_t len = isRaw ? n : cs, word = isRaw ? (n | 0x80000000u) : cs;
        const uint8_t* from = isRaw ? k->base + k->blkOffsets[b] : k->slots + (size_t)b * k->slot;
        uint64_t at;
        if (!fh_check_dev(e, sizeof *e, "frames pack: a block's frame entry")) return;
        at = e->cursor;
        k->offsets[b] = at;
        if (at <= e->limit && e->limit - at >= 4ull + len && fh_check_dev((uint8_t*)(uintptr_t)e->dst + at, 4 + (size_t)len, "frames pack: a record's place in its d_dst")
            && (!len || fh_check_dev(from, len, "frames pack: a record's source"))) {
            uint8_t* out = (uint8_t*)(uintptr_t)e->dst + at;
            out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
            if (len) memcpy(out + 4, from, len);
        }
        e->cursor = at + 4ull + len;
        if (e->cursor > e->limit) e->overflow = 1;
        e->rawRecords += (uint32_t)isRaw;
    }
}
int lzk_frames_pack_launch(const void* d_base, const uint64_t* d_blkOffsets, const uint32_t* d_blkSizes, const uint32_t* d_blkFrames,
                           const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, uint32_t nb,
                           LzFramesEntry* d_frames, hipStream_t stream)
{
    FramesPackK k;
    if (!d_base || !d_blkOffsets || !d_blkSizes || !d_blkFrames || !d_slots || !d_sizes || !d_offsets || !d_frames || nb == 0) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_frames_pack_launch: bad argument"); return -LIZARDGPU_ERR_ARG;
    }
    if (dfc_refused(0, "lzk_frames_pack_launch")) return -LIZARDGPU_ERR_HIP;
    k.base = (const uint8_t*)d_base; k.blkOffsets = d_blkOffsets; k.blkSizes = d_blkSizes; k.blkFrames = d_blkFrames; k.slots = (const uint8_t*)d_slots;
    k.slot = slot; k.sizes = d_sizes; k.offsets = d_offsets; k.nb = nb; k.frames = d_frames;
    return fh_enqueue_kernel(stream, frames_pack_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- lz_xxh32_frames_kernel ---- */
int lzk_frames_hash_launch(LzFramesEntry* d_frames, uint32_t nFrames, hipStream_t stream) { return dfc_frames_hash_launch(d_frames, nFrames, stream); }

/* ---- lz_frames_finish_kernel ---- */
typedef struct { const LzFramesEntry* frames; LzFramesResult* results; uint32_t n; } FramesFinishK;
static void frames_finish_kernel(void* a)
{
    const FramesFinishK* k = (const FramesFinishK*)a;
    uint32_t f, i;
    if (!fh_check_dev(k->frames, (size_t)k->n * sizeof *k->frames, "frames finish: the frame table")
        || !fh_check_dev(k->results, (size_t)k->n * sizeof *k->results, "frames finish: the result records")) return;
    for (f = 0; f < k->n; f++) {
        const LzFramesEntry* e = k->frames + f;
        LzFramesResult r = { 0, 0, 0 };
        if (e->flags & LZK_FRAMES_LIVE) {
            uint8_t* dst = (uint8_t*)(uintptr_t)e->dst;
            const size_t tail = e->flags & LZK_FRAMES_CHECKSUM ? 8 : 4;
            if (!fh_check_dev(dst, e->headerBytes, "frames finish: a frame's header")) continue;
            memcpy(dst, e->header, e->headerBytes);
            r.rawRecords = e->rawRecords;
            if (e->overflow || e->cursor > e->limit) r.size = LZK_FRAMES_OVERFLOW;
            else {
                if (!fh_check_dev(dst + e->cursor, tail, "frames finish: a frame's end mark and checksum")) continue;
                memset(dst + e->cursor, 0, 4);
                for (i = 0; i < 4 && tail == 8; i++) dst[e->cursor + 4 + i] = (uint8_t)(e->hash >> (8 * i));
                r.size = e->cursor + tail;
            }
        }
        k->results[f] = r;
    }
}
int lzk_frames_finish_launch(const LzFramesEntry* d_frames, LzFramesResult* d_results, uint32_t nFrames, hipStream_t stream)
{
    FramesFinishK k;
    if (!d_frames || !d_results || nFrames == 0) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_frames_finish_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    k.frames = d_frames; k.results = d_results; k.n = nFrames;
    return fh_enqueue_kernel(stream, frames_finish_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- one batch against the host twin, frame by frame ---- */
void pf_set_chunk_bytes(size_t n);
void pf_shutdown(void);
#define CHECK(cond, ...) DFC_CHECK("frames_device_fake", cond, __VA_ARGS__)
#define FDF_MAX 16
#define FDF_BLOCK ((size_t)131072)
#define FDF_DATA (12 * FDF_BLOCK)
static uint8_t* g_data;
const char* fdf_last_error(void) { return dfc_text; }            /* LizardGPU_lastError as the last batch left it (the twins' calls come behind it) */

/* P50 with noise across block borders, so that raw records lie between compressed ones */
static const uint8_t* fdf_data(void)
{
    if (!g_data) {
        unsigned long long x = 0x9E3779B97F4A7C15ull;
        size_t i;
        g_data = (uint8_t*)malloc(FDF_DATA);
        lzo_datagen(g_data, FDF_DATA, 0.5, 0.0, 77u);
        for (i = 2 * FDF_BLOCK - 5000; i < 3 * FDF_BLOCK + 4000; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; g_data[i] = (uint8_t)(x >> 32); }
        for (i = 9 * FDF_BLOCK; i < 10 * FDF_BLOCK; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; g_data[i] = (uint8_t)(x >> 32); }
    }
    return g_data;
}

/* Frame i: sizes[i] bytes of the data from offs[i], capacity = its bound + capDeltas[i].  Sources and destinations are fake device
 * allocations with 4 KiB canary margins, uploaded on a caller's stream that is not waited for; source i starts i % 4 bytes off the
 * margin.  wantRc: what the call must return; 0: every results[i] and every frame equal LizardGPU_compressFrame's, and a frame that
 * is refused below its bound leaves its region untouched; else every results[i] is GENERIC.  failMalloc: the n-th hipMalloc inside
 * the call fails.  grown (may be NULL): the growth of LizardGPU_frameCompressDeviceStats over the call. */
int fdf_batch(size_t nf, const size_t* offs, const size_t* sizes, const long* capDeltas, int level, int bsid, int checksum, int csize,
              int failMalloc, int wantRc, unsigned long long grown[4])
{
    const uint8_t* const data = fdf_data();
    LizardF_preferences_t p;
    const hipStream_t user = dfc_user();
    Region src[FDF_MAX], dst[FDF_MAX];
    void* dsts[FDF_MAX]; const void* srcs[FDF_MAX];
    size_t caps[FDF_MAX], results[FDF_MAX], i, g;
    unsigned long long s0[4], s1[4];
    int rc, bad = 0;
    CHECK(nf <= FDF_MAX, "too many frames");
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)bsid; p.frameInfo.blockMode = (LizardF_blockMode_t)1;
    p.frameInfo.contentChecksumFlag = (LizardF_contentChecksum_t)checksum; p.compressionLevel = level;
    for (i = 0; i < nf; i++) {
        const size_t n = sizes[i];
        CHECK(offs[i] + n <= FDF_DATA, "a frame outside the data");
        p.frameInfo.contentSize = csize ? n : 0;
        caps[i] = (size_t)((long)LizardGPU_compressFrameBound(n, &p) + capDeltas[i]);
        CHECK(!region_make(&src[i], data + offs[i], n, i % 4, 0x5A) && !region_make(&dst[i], NULL, caps[i], 0, 0xC3), "allocation");
        srcs[i] = region_at(&src[i]); dsts[i] = region_at(&dst[i]); results[i] = 12345;
    }
    p.frameInfo.contentSize = csize ? 1 : 0;                /* (not zero: every frame writes its own size) */
    if (failMalloc) hipStreamSynchronize(user);          /* (a call that fails before it orders itself behind the caller's stream leaves that stream's work queued, as it may) */
    memcpy(s0, lzk_ctx_peek()->devFrameCompressStats, sizeof s0);      /* (what LizardGPU_frameCompressDeviceStats of lizard_frame_device.c reads) */
    fh_fail_malloc(failMalloc);
    rc = LizardGPU_compressFrames_device(nf, dsts, caps, srcs, sizes, results, &p, user);
    fh_fail_malloc(0);
    dfc_keep_text();
    memcpy(s1, lzk_ctx_peek()->devFrameCompressStats, sizeof s1);
    for (g = 0; g < 4 && grown; g++) grown[g] = s1[g] - s0[g];
    hipStreamSynchronize(user);                          /* (a call that refused every frame up front never touched the caller's stream) */
    for (i = 0; i < nf && !bad; i++) {
        const size_t n = sizes[i];
        uint8_t* twin = (uint8_t*)malloc(caps[i] + 1);
        size_t t, q;
        p.frameInfo.contentSize = csize ? n : 0;
        t = LizardGPU_compressFrame(twin, caps[i], data + offs[i], n, &p);
        if (region_fetch(&dst[i]) || region_fetch_same(&src[i], data + offs[i])) bad = 1;
        if (!bad && (wantRc ? results[i] != LZ_FRAME_E(GENERIC) : results[i] != t)) bad = 2;
        if (!bad && !wantRc && !LizardF_isError(t) && memcmp(region_bytes(&dst[i]), twin, t)) bad = 3;
        if (!bad && !wantRc && capDeltas[i] < 0) for (q = 0; q < caps[i]; q++) if (region_bytes(&dst[i])[q] != 0xC3) bad = 4;
        free(twin);
        if (bad) fprintf(stderr, "frames_device_fake: frame %zu of %zu: %s (result %zu, twin %zu; n %zu level %d checksum %d csize %d cap %zu; call returned %d): %s\n", i, nf,
                         bad == 1 ? "a canary margin or the source changed" : bad == 2 ? "unexpected result" : bad == 3 ? "frame bytes differ from the twin's"
                         : "a frame refused below its bound was written to", results[i], t, n, level, checksum, csize, caps[i], rc, dfc_text);
    }
    for (i = 0; i < nf; i++) { region_free(&src[i]); region_free(&dst[i]); }
    CHECK(!bad, "a frame of the batch is wrong");
    CHECK(rc == wantRc, "the call returned %d, wanted %d: %s", rc, wantRc, dfc_text);
    return 0;
}

#ifdef FRAMES_DEVICE_FAKE_MAIN
/* ---- the program form, for the sanitizer build: batches over schedules, chunkings, checksum, levels, refusals and failures ---- */
int main(void)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 }, { FH_RANDOM, 12 }, { FH_RANDOM, 13 } };
    static const char* const chunk[] = { "1", "2", NULL, "4", "1" };
    const size_t bs = FDF_BLOCK;
    /* 3, 1, 0, 2 and 5 blocks, one byte, one block and a byte */
    const size_t offs[7] = { 0, 3 * bs, 0, 4 * bs, 6 * bs, 777, 9 * bs - 1 }, sizes[7] = { 3 * bs, bs, 0, 2 * bs, 5 * bs, 1, bs + 1 };
    const long atBound[7] = { 0, 0, 0, 0, 0, 0, 0 }, oneBelow[7] = { 0, 77, 0, -1, 0, 0, 0 };
    unsigned long long grown[4];
    size_t s;
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++) {
        const int checksum = (int)(s & 1), level = s & 2 ? 30 : 10;
        fh_set_schedule(sched[s].mode, sched[s].seed);
        pf_set_chunk_bytes((size_t)256 << 10);                        /* unset: two blocks per chunk */
        if (chunk[s]) setenv("LIZARDGPU_FRAME_CHUNK_BLOCKS", chunk[s], 1); else unsetenv("LIZARDGPU_FRAME_CHUNK_BLOCKS");
        if (s == 1) pf_shutdown();
        if (fdf_batch(7, offs, sizes, atBound, level, 1, checksum, 0, 0, 0, grown)) return 1;
        CHECK(grown[0] + grown[1] == 14 && grown[3] == 0, "statistics: %llu + %llu blocks, %llu source bytes on the host", grown[0], grown[1], grown[3]);
        if (fdf_batch(7, offs, sizes, atBound, level, 1, !checksum, 1, 0, 0, NULL)) return 1;       /* (the 1-byte frames answer dstMaxSize_tooSmall, as the twin) */
        if (fdf_batch(7, offs, sizes, oneBelow, level, 1, checksum, 0, 0, 0, NULL)) return 1;
        if (fdf_batch(7, offs, sizes, atBound, 18, 1, checksum, 0, 0, 0, grown)) return 1;
        CHECK(grown[2] == 0, "a batch of level 18 launched a chunk");
        /* a refused launch, a failing allocation (fresh stages: one of the first hipMallocs of the call); then a good call */
        pf_refuse_frames_pack(s & 1 ? 2 : 1);
        if (fdf_batch(5, offs, sizes, atBound, level, 1, checksum, 0, 0, -LIZARDGPU_ERR_HIP, NULL)) return 1;
        pf_shutdown();
        if (fdf_batch(5, offs, sizes, atBound, level, 1, checksum, 0, 1 + (int)(s % 3), -LIZARDGPU_ERR_NOMEM, NULL)) return 1;
        if (fdf_batch(5, offs, sizes, atBound, level, 1, checksum, 0, 0, 0, NULL)) return 1;
    }
    unsetenv("LIZARDGPU_FRAME_CHUNK_BLOCKS");
    printf("frames_device_fake: ok, %llu ops\n", fh_ops_run());
    return 0;
}
#endif
