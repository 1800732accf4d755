/* tests/unstream_device_fake.c — TEST INFRASTRUCTURE: lizard_amd/csrc/lizard_unstream_device.c (LizardGPU_decompressStream_device /
 * LizardGPU_streamIndex_device: the stream walk in segments, one host wait each, runs of frames with known sizes handed to the batch
 * decoder, the first frame a batch does not settle handed to the single-frame entry) compiled as a unit under test on a CPU, on the
 * fake HIP runtime with DEFERRED streams.  Linked with tests/unframes_device_fake.c (the batch decoder and its launches on the same
 * fake), tests/pipeline_fake.c (the context, the single-frame entry, the emulator's record decoder and walk) and tests/fake_hip.c as
 * they are; this file adds the one launch they do not have: lz_unstream_walk_kernel as a closure that checks that everything it
 * touches lies in live device memory and then runs the kernel's real body on the SIMT emulator (tests/unstream_fake_emul.cpp).
 * The unit's calls of LizardGPU_decompressFrames_device and LizardGPU_decompressFrame_device go through two spies that note their
 * arguments (relative to the stream and the destination of the run) and pass them on unchanged: usf_log() is what a test reads to
 * check how the stream was split into batches, which capacity every frame got and what the hand-over looked like.
 * usf_run decodes one caller-given stream and compares the answer — return value, consumed bytes, frame count, decoded count, the
 * decoded bytes — with the LOOP over LizardGPU_decompressFrame_device on the same fake, which is the entry's contract.
 *   library : with the files above, -shared (tests/test_stream_decompress_fake_device.py drives it through ctypes)
 *   program : -DUNSTREAM_DEVICE_FAKE_MAIN, for the sanitizer build: argv[1] = tests/golden/frame_ref_linked.liz; exit 0 = all good */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define LizardGPU_decompressFrames_device usf_spy_frames
#define LizardGPU_decompressFrame_device usf_spy_single
#include "../lizard_amd/csrc/lizard_unstream_device.c"     /* unit under test, compiled into this harness */
#undef LizardGPU_decompressFrames_device
#undef LizardGPU_decompressFrame_device
int LizardGPU_decompressFrames_device(size_t nFrames, void* const* d_dsts, const size_t* dstCapacities, const void* const* d_srcs,
                                      const size_t* srcSizes, size_t* results, size_t* srcConsumed, unsigned flags, void* stream);
size_t LizardGPU_decompressFrame_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr,
                                        unsigned flags, void* stream);
#include "device_fake_common.h"
#include "lizard_oracle.h"

void emul_unstream_segment(const void* src, unsigned long long srcSize, void* ctl, void* res, unsigned long long* offs, unsigned tableCap,
                           unsigned seed);                                                                      /* tests/unstream_fake_emul.cpp */

/* ---- the spies ---- */
#define USF_LOG 8192
static unsigned long long g_log[USF_LOG];
static size_t g_logN;
static const uint8_t *g_src0, *g_dst0;                        /* what the offsets of the log are relative to */
static void put(unsigned long long v) { if (g_logN < USF_LOG) g_log[g_logN++] = v; }
/* the log of the last usf_run: a batch is 1, n, then (srcOffset, srcSize, dstOffset, capacity) per frame, then flags; a hand-over is
 * 2, srcOffset, srcSize, dstOffset, capacity, flags */
size_t usf_log(unsigned long long* out, size_t room) { size_t i; for (i = 0; i < g_logN && i < room; i++) out[i] = g_log[i]; return g_logN; }

int usf_spy_frames(size_t nFrames, void* const* d_dsts, const size_t* dstCapacities, const void* const* d_srcs, const size_t* srcSizes,
                   size_t* results, size_t* srcConsumed, unsigned flags, void* stream)
{
    size_t i;
    put(1); put(nFrames);
    for (i = 0; i < nFrames; i++) {
        put((unsigned long long)((const uint8_t*)d_srcs[i] - g_src0)); put(srcSizes[i]);
        put((unsigned long long)((const uint8_t*)d_dsts[i] - g_dst0)); put(dstCapacities[i]);
    }
    put(flags);
    return LizardGPU_decompressFrames_device(nFrames, d_dsts, dstCapacities, d_srcs, srcSizes, results, srcConsumed, flags, stream);
}

size_t usf_spy_single(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr, unsigned flags, void* stream)
{
    put(2); put((unsigned long long)((const uint8_t*)d_src - g_src0)); put(srcSize);
    put((unsigned long long)((const uint8_t*)d_dst - g_dst0)); put(dstCapacity); put(flags);
    return LizardGPU_decompressFrame_device(d_dst, dstCapacity, d_src, srcSize, srcConsumedPtr, flags, stream);
}

/* ---- lz_unstream_walk_kernel ---- */
void usf_refuse(int nth) { dfc_refuse_set(0, nth); }      /* the n-th stream walk launch from now answers -LIZARDGPU_ERR_HIP, once */

typedef struct { const uint8_t* src; uint64_t srcSize; LzStreamCtl* ctl; LzWalkResult* res; uint64_t* offs; uint32_t cap; } StreamK;
static void stream_kernel(void* a)
{
    const StreamK* k = (const StreamK*)a;
    if (!fh_check_dev(k->ctl, sizeof *k->ctl, "stream walk: the control record") || !fh_check_dev(k->src, (size_t)k->srcSize, "stream walk: src[0..srcSize)")
        || !fh_check_dev(k->res, (size_t)k->cap * sizeof *k->res, "stream walk: the result table") || !fh_check_dev(k->offs, 8 * (size_t)k->cap, "stream walk: the offset table")) return;
    emul_unstream_segment(k->src, k->srcSize, k->ctl, k->res, (unsigned long long*)k->offs, k->cap, fh_rand() | 1u);
}
int lzk_unstream_walk_launch(const void* d_src, size_t srcSize, LzStreamCtl* d_ctl, LzWalkResult* d_res, uint64_t* d_offs, uint32_t tableCap, hipStream_t stream)
{
    StreamK k;
    if (!d_src || !d_ctl || !d_res || !d_offs || tableCap == 0) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_unstream_walk_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    if (dfc_refused(0, "lzk_unstream_walk_launch")) return -LIZARDGPU_ERR_HIP;
    k.src = (const uint8_t*)d_src; k.srcSize = srcSize; k.ctl = d_ctl; k.res = d_res; k.offs = d_offs; k.cap = tableCap;
    return fh_enqueue_kernel(stream, stream_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- one stream against the loop over the single-frame entry ---- */
void pf_shutdown(void);
#define CHECK(cond, ...) DFC_CHECK("unstream_device_fake", cond, __VA_ARGS__)
const char* usf_last_error(void) { return dfc_text; }           /* LizardGPU_lastError as the entry left it */

/* The stream `bytes` (n of them) decoded into cap bytes.  The source starts skew bytes (0 - 7) off an aligned address.  wantGeneric 0:
 * the entry's four answers and the bytes d_dst[0 .. decoded) must be the loop's; 1: the machinery is made to fail by the caller
 * (usf_refuse, udf_refuse, failMalloc: the n-th hipMalloc inside the call), the entry must answer GENERIC with a text.
 * got (may be NULL): return value, consumed, frames, decoded, then the growth of LizardGPU_streamDecodeDeviceStats [0..3]. */
int usf_run(const uint8_t* bytes, size_t n, size_t cap, unsigned flags, unsigned skew, int failMalloc, int wantGeneric, unsigned long long got[8])
{
    Region src, dst, one;
    unsigned long long s0[4], s1[4];
    size_t r, used = 12345, frames = 12345, decoded = 12345, pos = 0, out = 0, count = 0, answer;
    const hipStream_t user = dfc_user();
    int bad = 0, g;
    CHECK(!region_make(&src, bytes, n, skew & 7, 0x5A) && !region_make(&dst, NULL, cap, (skew * 3) & 7, 0xC3), "allocation");
    if (failMalloc) hipStreamSynchronize(user);
    g_logN = 0; g_src0 = region_at(&src); g_dst0 = region_at(&dst);
    LizardGPU_streamDecodeDeviceStats(s0);
    fh_fail_malloc(failMalloc);
    r = LizardGPU_decompressStream_device(region_at(&dst), cap, region_at(&src), n, &used, &frames, &decoded, flags, user);
    fh_fail_malloc(0);
    dfc_keep_text();
    LizardGPU_streamDecodeDeviceStats(s1);
    hipStreamSynchronize(user);
    if (got) { got[0] = r; got[1] = used; got[2] = frames; got[3] = decoded; for (g = 0; g < 4; g++) got[4 + g] = s1[g] - s0[g]; }
    if (region_fetch_same(&src, bytes) || region_fetch(&dst)) bad = 1;
    /* the loop */
    CHECK(!region_make(&one, NULL, cap, (skew * 3) & 7, 0xC3), "allocation");
    answer = 0;
    while (!bad && pos < n) {
        size_t u = 777;
        const size_t t = LizardGPU_decompressFrame_device(region_at(&one) + out, cap - out, region_at(&src) + pos, n - pos, &u, flags, user);
        hipStreamSynchronize(user);
        if (LizardGPU_frameIsError(t)) { answer = t; break; }
        out += t; pos += u; count++;
    }
    if (!answer) answer = out;
    hipStreamSynchronize(user);
    if (!bad && region_fetch(&one)) bad = 5;
    if (!bad && wantGeneric) {
        if (r != LZ_FRAME_E(GENERIC) || !dfc_text[0]) bad = 6;
        else if (frames > count || decoded > out || (decoded && memcmp(region_bytes(&dst), region_bytes(&one), decoded))) bad = 3;
    }
    if (!bad && !wantGeneric && (r != answer || used != pos || frames != count || decoded != out)) bad = 2;
    if (!bad && !wantGeneric && out && memcmp(region_bytes(&dst), region_bytes(&one), out)) bad = 3;
    if (bad) fprintf(stderr, "unstream_device_fake: %s (entry: %zu, consumed %zu, %zu frames, %zu decoded; loop: %zu, consumed %zu, %zu frames, %zu decoded; %zu bytes, cap %zu, flags %u): %s\n",
                     bad == 1 ? "a canary margin or the source changed" : bad == 2 ? "the answer differs from the loop's" : bad == 3 ? "decoded bytes differ from the loop's"
                     : bad == 5 ? "the single entry wrote outside its d_dst" : "a failure of the machinery was not answered GENERIC with a text",
                     r, used, frames, decoded, answer, pos, count, out, n, cap, flags, dfc_text);
    region_free(&src); region_free(&dst); region_free(&one);
    return bad;
}

/* LizardGPU_streamIndex_device over the stream: the arrays come back as they are; returns the code */
int usf_index(const uint8_t* bytes, size_t n, unsigned skew, uint64_t* offs, uint64_t* fbytes, LizardGPU_frameInfo_t* infos, size_t* nrec, size_t maxFrames,
              size_t* nFrames, size_t* streamBytes)
{
    Region src;
    int rc;
    if (region_make(&src, bytes, n, skew & 7, 0x5A)) return 1000;
    rc = LizardGPU_streamIndex_device(region_at(&src), n, offs, fbytes, infos, nrec, maxFrames, nFrames, streamBytes, dfc_user());
    dfc_keep_text();
    hipStreamSynchronize(dfc_user());
    if (region_fetch(&src)) rc = 1001;
    region_free(&src);
    return rc;
}

#ifdef UNSTREAM_DEVICE_FAKE_MAIN
/* ---- the program form, for the sanitizer build: streams made here, over schedules, capacities, segment sizes, refusals and failures ---- */
void fh_set_schedule(int mode, unsigned seed);
void udf_refuse(int kind, int nth);                            /* tests/unframes_device_fake.c */
#define BLK ((size_t)131072)
static uint8_t* g_data;
static size_t make_frame(uint8_t* out, size_t cap, size_t off, size_t n, int level, int checksum, int csize)
{
    LizardF_preferences_t p;
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)1; p.frameInfo.blockMode = (LizardF_blockMode_t)1;
    p.frameInfo.contentChecksumFlag = (LizardF_contentChecksum_t)checksum; p.frameInfo.contentSize = csize ? n : 0; p.compressionLevel = level;
    return LizardGPU_compressFrame(out, cap, g_data + off, n, &p);
}

int main(int argc, char** argv)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 }, { FH_RANDOM, 12 } };
    static const uint8_t skippable[] = { 0x57, 0x2A, 0x4D, 0x18, 5, 0, 0, 0, 's', 'k', 'i', 'p', '!' };
    static const size_t plain[4] = { BLK + 5000, 70000, 0, 1 };
    uint8_t *pool = (uint8_t*)malloc(16 * BLK), *st = (uint8_t*)malloc(16 * BLK), *golden = NULL;
    size_t goldenBytes = 0, s;
    unsigned long long got[8];
    g_data = (uint8_t*)malloc(4 * BLK);
    lzo_datagen(g_data, 4 * BLK, 0.5, 0.0, 77u);
    if (argc > 1) {
        FILE* fp = fopen(argv[1], "rb");
        CHECK(fp, "cannot open %s", argv[1]);
        golden = (uint8_t*)malloc(4 * BLK);
        goldenBytes = fread(golden, 1, 4 * BLK, fp); fclose(fp);
        CHECK(goldenBytes > 15 && goldenBytes < 4 * BLK, "golden frame");
    }
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++) {
        const int checksum = (int)(s & 1), level = s & 2 ? 30 : 10;
        size_t f[4], fn[4], n, total = 0, first2, i, at = 0;
        fh_set_schedule(sched[s].mode, sched[s].seed);
        if (s == 1) pf_shutdown();
        for (i = 0; i < 4; i++) {                              /* with content size, and without */
            f[i] = make_frame(pool + at, 16 * BLK - at, i * 1000, plain[i], level, checksum, 1); CHECK(!LizardF_isError(f[i]), "frame"); at += f[i];
            total += plain[i];
        }
        for (i = 0; i < 2; i++) { fn[i] = make_frame(pool + at, 16 * BLK - at, 30000 + i, plain[i], level, checksum, 0); CHECK(!LizardF_isError(fn[i]), "frame"); at += fn[i]; }
        first2 = plain[0] + plain[1];
        /* every frame sized, a skippable one in the middle: ONE batch, no hand-over */
        n = f[0] + f[1]; memcpy(st, pool, n); memcpy(st + n, skippable, sizeof skippable); n += sizeof skippable; memcpy(st + n, pool + f[0] + f[1], f[2] + f[3]); n += f[2] + f[3];
        setenv("LIZARDGPU_STREAM_WALK_FRAMES", s & 1 ? "2" : "4096", 1);
        if (usf_run(st, n, total, 0, (unsigned)s, 0, 0, got)) return 1;
        CHECK(got[0] == total && got[1] == n && got[2] == 5 && got[5] == 1 && got[6] == 0 && got[7] == (s & 1 ? 3u : 1u), "one batch: %llu %llu %llu, %llu batches, %llu handed over, %llu segments", got[0], got[1], got[2], got[5], got[6], got[7]);
        if (usf_run(st, n, total - 1, LIZARDGPU_FRAME_SKIP_CHECKSUM, 3, 0, 0, got)) return 1;
        CHECK(LizardGPU_frameIsError((size_t)got[0]) && got[2] == 4 && got[3] == total - 1 && got[6] == 1, "one byte short");
        if (usf_run(st, n, first2, 0, 1, 0, 0, got) || usf_run(st, n, 0, 0, 0, 0, 0, got)) return 1;
        if (usf_run(st, n - 1, total, 0, 5, 0, 0, got) || usf_run(st, n - 5, total, 0, 2, 0, 0, got)) return 1;
        /* frames without content size between sized ones, the linked frame of the reference, garbage at the end */
        at = f[0] + f[1] + f[2] + f[3];
        n = 0; memcpy(st + n, pool + at, fn[0]); n += fn[0]; memcpy(st + n, pool, f[0]); n += f[0]; memcpy(st + n, pool + at + fn[0], fn[1]); n += fn[1];
        if (golden) { memcpy(st + n, golden, goldenBytes); n += goldenBytes; }
        memcpy(st + n, pool + f[0], f[1]); n += f[1];
        if (usf_run(st, n, 32 * BLK, 0, 7, 0, 0, got)) return 1;
        CHECK(got[2] == (golden ? 5u : 4u) && got[6] == (golden ? 1u : 0u) && got[5] == 3u, "mixed stream: %llu frames, %llu batches, %llu handed over", got[2], got[5], got[6]);
        memcpy(st + n, "\xde\xad\xbe\xef", 4);
        if (usf_run(st, n + 4, 32 * BLK, 0, 6, 0, 0, got)) return 1;
        CHECK(got[0] == LZ_FRAME_E(frameHeader_incomplete) && got[1] == n, "garbage at the end");
        /* the machinery fails, then a good call */
        usf_refuse(1);
        if (usf_run(st, n, 32 * BLK, 0, 0, 0, 1, NULL)) return 1;
        udf_refuse((int)(s % 4), 1);
        if (usf_run(st, n, 32 * BLK, 0, 0, 0, 1, NULL)) return 1;
        pf_shutdown();
        if (usf_run(st, n, 32 * BLK, 0, 0, 1, 1, NULL)) return 1;
        if (usf_run(st, n, 32 * BLK, 0, 0, 0, 0, NULL)) return 1;
    }
    unsetenv("LIZARDGPU_STREAM_WALK_FRAMES");
    free(pool); free(st); free(golden); free(g_data);
    printf("unstream_device_fake: ok, %llu ops\n", fh_ops_run());
    return 0;
}
#endif
