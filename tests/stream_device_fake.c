/* tests/stream_device_fake.c — TEST INFRASTRUCTURE: lizard_amd/csrc/lizard_stream_device.c (LizardGPU_compressStream_device: the blocks of
 * many frames as one list of chunks enqueued up front on three streams, the stages' slots rotating under events, ONE carry word in
 * device memory from which every record's place in the one destination follows, prefixes, heads and tails written by a kernel)
 * compiled as a unit under test on a CPU, on the fake HIP runtime with DEFERRED streams.  Linked with tests/pipeline_fake.c (the
 * context, lzk_launch = the oracle as the block kernels over a ragged batch, the host twin LizardGPU_compressFrame on the same fake)
 * and tests/fake_hip.c as they are; this file adds the shims they do not have: plain sequential models of lz_stream_scan_kernel +
 * lz_frames_gather_kernel, lz_xxh32_frames_kernel and lz_stream_finish_kernel (lz_stream_pack.h, lz_frames_pack.h) that check that
 * everything they touch lies in live device memory.
 * sdf_refuse_pack: the n-th pack launch from now answers -LIZARDGPU_ERR_HIP, once, and enqueues nothing.
 * sdf_batch runs one call and compares the stream with prefix + LizardGPU_compressFrame per frame on the same bytes; both forms have it.
 *   library : with pipeline_fake.c, -shared (tests/test_stream_compress_fake_device.py drives it through ctypes)
 *   program : -DSTREAM_DEVICE_FAKE_MAIN, for the sanitizer build: exit 0 = all good */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../lizard_amd/csrc/lizard_stream_device.c"       /* unit under test, compiled into this harness */
#include "device_fake_common.h"
#include "lizard_oracle.h"

void sdf_refuse_pack(int nth) { dfc_refuse_set(0, nth); }

/* ---- lz_stream_scan_kernel + lz_frames_gather_kernel: block after block, the carry advancing as the records are placed ---- */
typedef struct { const uint8_t* base; const uint64_t* blkOffsets; const uint32_t *blkSizes, *blkFrames; const uint8_t* slots; size_t slot;
                 const uint32_t* sizes; uint64_t* offsets; uint32_t nb, first; const LzFramesEntry* frames; LzStreamEntry* entries;
                 LzStreamState* state; uint64_t capacity; } StreamPackK;
static void stream_pack_kernel(void* a)
{
    const StreamPackK* k = (const StreamPackK*)a;
    uint32_t b;
    if (!fh_check_dev(k->sizes, 4 * (size_t)k->nb, "stream pack: sizes") || !fh_check_dev(k->offsets, 8 * (size_t)k->nb, "stream pack: offsets")
        || !fh_check_dev(k->blkOffsets, 8 * (size_t)k->nb, "stream pack: block offsets") || !fh_check_dev(k->blkSizes, 4 * (size_t)k->nb, "stream pack: block sizes")
        || !fh_check_dev(k->blkFrames, 4 * (size_t)k->nb, "stream pack: block frames") || !fh_check_dev(k->state, sizeof *k->state, "stream pack: the state")) return;
    for (b = 0; b < k->nb; b++) {
        const LzFramesEntry* f = k->frames + k->blkFrames[b];
        LzStreamEntry* e = k->entries + k->blkFrames[b];
        const uint32_t n = k->blkSizes[b], cs = k->sizes[b], g = k->first + b;
        const int isRaw = n != 1u && (cs == 0u || cs > n - 1u);
        const uint32_t len = isRaw ? n : cs, word = isRaw ? (n | 0x80000000u) : cs;
        const uint8_t* from = isRaw ? k->base + k->blkOffsets[b] : k->slots + (size_t)b * k->slot;
        uint64_t at;
        if (!fh_check_dev(f, sizeof *f, "stream pack: a block's frame entry") || !fh_check_dev(e, sizeof *e, "stream pack: a block's stream entry")) return;
        if (g == e->firstBlock) e->before = k->state->carry;
        at = e->fixed + k->state->carry;
        k->offsets[b] = at;
        if (at <= f->limit && f->limit - at >= 4ull + len && fh_check_dev((uint8_t*)(uintptr_t)f->dst + at, 4 + (size_t)len, "stream pack: a record's place in d_dst")
            && (!len || fh_check_dev(from, len, "stream pack: a record's source"))) {
            uint8_t* out = (uint8_t*)(uintptr_t)f->dst + at;
            out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
            if (len) memcpy(out + 4, from, len);
        }
        k->state->carry += 4ull + len;
        if (e->fixed + k->state->carry + (g == e->lastBlock ? e->tailBytes : 0u) > k->capacity) k->state->overflow = 1;
        k->state->rawRecords += (uint32_t)isRaw;
    }
}
int lzk_stream_pack_launch(const void* d_base, const uint64_t* d_blkOffsets, const uint32_t* d_blkSizes, const uint32_t* d_blkFrames,
                           const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, uint32_t nb, uint32_t firstBlock,
                           const LzFramesEntry* d_frames, LzStreamEntry* d_entries, LzStreamState* d_state, uint64_t capacity, hipStream_t stream)
{
    StreamPackK k;
    if (!d_base || !d_blkOffsets || !d_blkSizes || !d_blkFrames || !d_slots || !d_sizes || !d_offsets || !d_frames || !d_entries || !d_state || nb == 0) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_stream_pack_launch: bad argument"); return -LIZARDGPU_ERR_ARG;
    }
    if (dfc_refused(0, "lzk_stream_pack_launch")) return -LIZARDGPU_ERR_HIP;
    k.base = (const uint8_t*)d_base; k.blkOffsets = d_blkOffsets; k.blkSizes = d_blkSizes; k.blkFrames = d_blkFrames; k.slots = (const uint8_t*)d_slots;
    k.slot = slot; k.sizes = d_sizes; k.offsets = d_offsets; k.nb = nb; k.first = firstBlock; k.frames = d_frames; k.entries = d_entries; k.state = d_state;
    k.capacity = capacity;
    return fh_enqueue_kernel(stream, stream_pack_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- lz_xxh32_frames_kernel ---- */
int lzk_frames_hash_launch(LzFramesEntry* d_frames, uint32_t nFrames, hipStream_t stream) { return dfc_frames_hash_launch(d_frames, nFrames, stream); }

/* ---- lz_stream_finish_kernel ---- */
typedef struct { const LzFramesEntry* frames; const LzStreamEntry* entries; const uint8_t* blob; const LzStreamState* state; uint32_t n;
                 uint64_t fixedTotal, capacity; LzFramesResult* result; uint64_t* offsets; } StreamFinishK;
static void stream_finish_kernel(void* a)
{
    const StreamFinishK* k = (const StreamFinishK*)a;
    uint64_t total, carry;
    uint32_t f, i;
    int over;
    if (!fh_check_dev(k->frames, (size_t)k->n * sizeof *k->frames, "stream finish: the frame table")
        || !fh_check_dev(k->entries, (size_t)k->n * sizeof *k->entries, "stream finish: the stream table")
        || !fh_check_dev(k->state, sizeof *k->state, "stream finish: the state") || !fh_check_dev(k->result, sizeof *k->result, "stream finish: the result record")
        || !fh_check_dev(k->offsets, 8 * ((size_t)k->n + 1), "stream finish: the frame offsets")) return;
    carry = k->state->carry; total = k->fixedTotal + carry;
    over = k->state->overflow || total > k->capacity;
    k->result->size = over ? LZK_FRAMES_OVERFLOW : total; k->result->rawRecords = k->state->rawRecords; k->result->reserved = 0;
    k->offsets[k->n] = total;
    if (over) return;
    for (f = 0; f < k->n; f++) {
        const LzFramesEntry* e = k->frames + f;
        const LzStreamEntry* s = k->entries + f;
        const uint64_t before = s->nextSelf < k->n ? k->entries[s->nextSelf].before : carry, after = s->nextAfter < k->n ? k->entries[s->nextAfter].before : carry;
        const uint64_t start = s->fixed - e->headerBytes - s->prefixBytes + before;
        uint8_t* dst = (uint8_t*)(uintptr_t)e->dst;
        if (!fh_check_dev(dst + start, (size_t)s->prefixBytes + e->headerBytes, "stream finish: a frame's prefix and header")
            || (s->prefixBytes && !fh_check_dev(k->blob + s->prefixOff, (size_t)s->prefixBytes, "stream finish: a prefix in the blob"))
            || !fh_check_dev(dst + s->fixed + after, s->tailBytes, "stream finish: a frame's end mark and checksum")) continue;
        if (s->prefixBytes) memcpy(dst + start, k->blob + s->prefixOff, (size_t)s->prefixBytes);
        memcpy(dst + start + s->prefixBytes, e->header, e->headerBytes);
        memset(dst + s->fixed + after, 0, 4);
        for (i = 0; i < 4 && s->tailBytes == 8; i++) dst[s->fixed + after + 4 + i] = (uint8_t)(e->hash >> (8 * i));
        k->offsets[f] = start;
    }
}
int lzk_stream_finish_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const void* d_blob, const LzStreamState* d_state,
                             uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, LzFramesResult* d_result, uint64_t* d_offsets, hipStream_t stream)
{
    StreamFinishK k;
    if (!d_frames || !d_entries || !d_blob || !d_state || !d_result || !d_offsets || nFrames == 0) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_stream_finish_launch: bad argument"); return -LIZARDGPU_ERR_ARG;
    }
    k.frames = d_frames; k.entries = d_entries; k.blob = (const uint8_t*)d_blob; k.state = d_state; k.n = nFrames; k.fixedTotal = fixedTotal;
    k.capacity = capacity; k.result = d_result; k.offsets = d_offsets;
    return fh_enqueue_kernel(stream, stream_finish_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* ---- one call against prefix + the host twin, frame by frame ---- */
void pf_set_chunk_bytes(size_t n);
void pf_shutdown(void);
#define CHECK(cond, ...) DFC_CHECK("stream_device_fake", cond, __VA_ARGS__)
#define SDF_MAX 16
#define SDF_BLOCK ((size_t)131072)
#define SDF_DATA (12 * SDF_BLOCK)
enum { SDF_CAP_BOUND = 0, SDF_CAP_EXACT = 1, SDF_CAP_ONE_BELOW = 2 };
static uint8_t* g_data;
const char* sdf_last_error(void) { return dfc_text; }            /* LizardGPU_lastError as the last call left it (the twins' calls come behind it) */

/* P50 with noise across block borders, so that raw records lie between compressed ones; the block in front of 10 * SDF_BLOCK is noise */
static const uint8_t* sdf_data(void)
{
    if (!g_data) {
        unsigned long long x = 0x9E3779B97F4A7C15ull;
        size_t i;
        g_data = (uint8_t*)malloc(SDF_DATA);
        lzo_datagen(g_data, SDF_DATA, 0.5, 0.0, 77u);
        for (i = 2 * SDF_BLOCK - 5000; i < 3 * SDF_BLOCK + 4000; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; g_data[i] = (uint8_t)(x >> 32); }
        for (i = 9 * SDF_BLOCK; i < 10 * SDF_BLOCK; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; g_data[i] = (uint8_t)(x >> 32); }
    }
    return g_data;
}

/* a prefix of n bytes: from 8 bytes on a skippable frame, as a tensor header is one; shorter ones are just bytes */
static void sdf_prefix(uint8_t* p, size_t n, size_t i)
{
    size_t k;
    for (k = 0; k < n; k++) p[k] = (uint8_t)(0xA0 + 7 * i + k);
    if (n >= 8) {
        const uint32_t magic = 0x184D2A50u + (uint32_t)(i % 16), len = (uint32_t)(n - 8);
        for (k = 0; k < 4; k++) { p[k] = (uint8_t)(magic >> (8 * k)); p[4 + k] = (uint8_t)(len >> (8 * k)); }
    }
}

/* [from, to) of the stream through LizardF_decompress, call after call: the decoded bytes must be want[0 .. n) */
static int sdf_decode(const uint8_t* stream, size_t from, size_t to, const uint8_t* want, size_t n)
{
    LizardF_decompressionContext_t d = NULL;
    uint8_t* out = (uint8_t*)malloc(n + 1);
    size_t pos = from, got = 0, r = 1;
    int bad = 0;
    if (LizardF_isError(LizardF_createDecompressionContext(&d, 100))) { free(out); return 1; }
    while (pos < to && !bad) {
        size_t ds = n - got, ss = to - pos;
        r = LizardF_decompress(d, out + got, &ds, stream + pos, &ss, NULL);
        if (LizardF_isError(r) || (!ss && !ds)) bad = 1;
        pos += ss; got += ds;
    }
    if (!bad && (r != 0 || got != n || (n && memcmp(out, want, n)))) bad = 1;
    LizardF_freeDecompressionContext(d);
    free(out);
    return bad;
}

/* Frame i: sizes[i] bytes of the data from offs[i] behind a prefix of prefixSizes[i] bytes (NULL: no prefixes).  Sources and the
 * destination are fake device allocations with 4 KiB canary margins, uploaded on a caller's stream that is not waited for; source i
 * starts i % 4 bytes off the margin; the sources of the frames in nullMask are NULL.  capMode: SDF_CAP_*.  want: what the call must
 * return; 0: the stream's size, and then the bytes equal prefix + LizardGPU_compressFrame per frame, the offsets are right and
 * LizardF_decompress reads every [offset i, offset i + 1) back (when every prefix is empty or a skippable frame).  An up-front refusal
 * (wantFailed >= 0) must name that frame and leave d_dst untouched; every other answer must leave the margins alone.  failMalloc:
 * the n-th hipMalloc inside the call fails.  grown (may be NULL): the growth of LizardGPU_streamCompressDeviceStats and, in [4 .. 8),
 * of LizardGPU_frameCompressDeviceStats' counters over the call. */
int sdf_batch(size_t nf, const size_t* offs, const size_t* sizes, const size_t* prefixSizes, int level, int bsid, int blockMode, int checksum,
              int capMode, unsigned nullMask, int failMalloc, size_t want, long wantFailed, unsigned long long grown[8])
{
    const uint8_t* const data = sdf_data();
    LizardF_preferences_t p;
    const hipStream_t user = dfc_user();
    Region src[SDF_MAX], dst;
    uint8_t *prefix[SDF_MAX], *expect;
    const void *srcs[SDF_MAX], *prefixes[SDF_MAX];
    uint64_t offsets[SDF_MAX + 1], wantOffsets[SDF_MAX + 1];
    size_t i, q, g, total = 0, bound, cap, ret, failed = 777;
    unsigned long long s0[8], s1[8];
    int bad = 0, decodable = 1;
    CHECK(nf <= SDF_MAX, "too many frames");
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)bsid; p.frameInfo.blockMode = (LizardF_blockMode_t)blockMode;
    p.frameInfo.contentChecksumFlag = (LizardF_contentChecksum_t)checksum; p.compressionLevel = level;
    p.frameInfo.contentSize = 1;                            /* (not zero: every frame writes its own size) */
    bound = LizardGPU_compressStreamBound(nf, sizes, prefixSizes, &p);
    CHECK(!LizardF_isError(bound), "the bound is an error code");
    /* what the stream must be: prefix + the host twin's frame at bound + 8, when the call is to succeed or to miss its capacity */
    expect = (uint8_t*)malloc(bound + 1);
    for (i = 0; i < nf; i++) {
        const size_t pre = prefixSizes ? prefixSizes[i] : 0;
        prefix[i] = (uint8_t*)malloc(pre + 1); sdf_prefix(prefix[i], pre, i); prefixes[i] = prefix[i];
        if (pre && pre < 8) decodable = 0;
        wantOffsets[i] = total;
        if (wantFailed >= 0 || (want && want != LZ_FRAME_E(dstMaxSize_tooSmall))) continue;
        memcpy(expect + total, prefix[i], pre); total += pre;
        p.frameInfo.contentSize = sizes[i];
        q = LizardGPU_compressFrame(expect + total, LizardGPU_compressFrameBound(sizes[i], &p) + 8, data + offs[i], sizes[i], &p);
        p.frameInfo.contentSize = 1;
        if (LizardF_isError(q)) { fprintf(stderr, "stream_device_fake: the twin refused frame %zu: %s\n", i, LizardF_getErrorName(q)); bad = 9; break; }
        total += q;
    }
    wantOffsets[nf] = total;
    cap = capMode == SDF_CAP_BOUND ? bound : capMode == SDF_CAP_EXACT ? total : total - 1;
    for (i = 0; i < nf; i++) {
        CHECK(offs[i] + sizes[i] <= SDF_DATA, "a frame outside the data");
        CHECK(!region_make(&src[i], data + offs[i], sizes[i], i % 4, 0x5A), "allocation");
        srcs[i] = (nullMask >> i) & 1u ? NULL : region_at(&src[i]);
    }
    CHECK(!region_make(&dst, NULL, cap, 0, 0xC3), "allocation");
    if (failMalloc) hipStreamSynchronize(user);          /* (a call that fails before it orders itself behind the caller's stream leaves that stream's work queued, as it may) */
    memcpy(s0, lzk_ctx_peek()->devStreamCompressStats, 4 * sizeof s0[0]); memcpy(s0 + 4, lzk_ctx_peek()->devFrameCompressStats, 4 * sizeof s0[0]);
    for (i = 0; i <= nf; i++) offsets[i] = 0xDEADBEEFull;
    fh_fail_malloc(failMalloc);
    ret = LizardGPU_compressStream_device(region_at(&dst), cap, nf, srcs, sizes, prefixSizes ? prefixes : NULL, prefixSizes, &p, offsets, &failed, user);
    fh_fail_malloc(0);
    dfc_keep_text();
    memcpy(s1, lzk_ctx_peek()->devStreamCompressStats, 4 * sizeof s1[0]); memcpy(s1 + 4, lzk_ctx_peek()->devFrameCompressStats, 4 * sizeof s1[0]);
    for (g = 0; g < 8 && grown; g++) grown[g] = s1[g] - s0[g];
    hipStreamSynchronize(user);                          /* (a call that refused up front never touched the caller's stream) */
    if (region_fetch(&dst) && !bad) bad = 1;
    for (i = 0; i < nf && !bad; i++) if (region_fetch_same(&src[i], data + offs[i])) bad = 1;
    if (!bad && ret != (want ? want : total)) bad = 2;
    if (!bad && wantFailed >= 0 && failed != (size_t)wantFailed) bad = 5;
    if (!bad && wantFailed >= 0) for (q = 0; q < cap; q++) if (region_bytes(&dst)[q] != 0xC3) { bad = 6; break; }
    if (!bad && !want && memcmp(region_bytes(&dst), expect, total)) bad = 3;
    if (!bad && !want && memcmp(offsets, wantOffsets, 8 * (nf + 1))) bad = 4;
    for (i = 0; i < nf && !bad && !want && decodable; i++)
        if (sdf_decode(region_bytes(&dst), (size_t)offsets[i], (size_t)offsets[i + 1], data + offs[i], sizes[i])) bad = 7;
    if (bad) fprintf(stderr, "stream_device_fake: %s (returned %zu, wanted %zu, total %zu; frames %zu level %d checksum %d cap %zu bound %zu failed %zu): %s\n",
                     bad == 1 ? "a canary margin or a source changed" : bad == 2 ? "unexpected return value" : bad == 3 ? "stream bytes differ from prefix + the twins' frames"
                     : bad == 4 ? "wrong frame offsets" : bad == 5 ? "wrong failed frame" : bad == 6 ? "a call refused up front wrote to d_dst"
                     : bad == 7 ? "LizardF_decompress does not read a frame back" : "the twin refused", ret, want, total, nf, level, checksum, cap, bound, failed, dfc_text);
    for (i = 0; i < nf; i++) { region_free(&src[i]); free(prefix[i]); }
    region_free(&dst); free(expect);
    CHECK(!bad, "the call is wrong");
    return 0;
}

#ifdef STREAM_DEVICE_FAKE_MAIN
/* ---- the program form, for the sanitizer build: one pass of the batch per schedule, with the capacities, refusals and failures ---- */
int main(void)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 } };
    static const char* const chunk[] = { "1", NULL, "3" };
    const size_t bs = SDF_BLOCK;
    /* 3, 1, 0, 0, 2 and 5 blocks, one byte, one block and a byte, 0 */
    const size_t offs[9] = { 0, 3 * bs, 0, 0, 4 * bs, 6 * bs, 777, 9 * bs - 1, 0 }, sizes[9] = { 3 * bs, bs, 0, 0, 2 * bs, 5 * bs, 1, bs + 1, 0 };
    const size_t pre[9] = { 56, 0, 48, 64, 8, 56, 72, 56, 48 };
    const size_t lateOffs[4] = { 3 * bs, 0, 4 * bs, 6 * bs }, lateSizes[4] = { bs, 0, 2 * bs, 5 * bs };
    unsigned long long grown[8];
    size_t s;
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++) {
        const int checksum = (int)(s & 1), level = s & 2 ? 30 : 10;
        fh_set_schedule(sched[s].mode, sched[s].seed);
        pf_set_chunk_bytes((size_t)256 << 10);                        /* unset: two blocks per chunk */
        if (chunk[s]) setenv("LIZARDGPU_FRAME_CHUNK_BLOCKS", chunk[s], 1); else unsetenv("LIZARDGPU_FRAME_CHUNK_BLOCKS");
        if (s == 1) pf_shutdown();
        if (sdf_batch(9, offs, sizes, pre, level, 1, 1, checksum, SDF_CAP_BOUND, 0, 0, 0, -1, grown)) return 1;
        CHECK(grown[0] == 9 && grown[1] >= 2 && grown[3] == 1 && !grown[4] && !grown[5] && !grown[6], "statistics: %llu frames, %llu raw, %llu calls", grown[0], grown[1], grown[3]);
        if (sdf_batch(9, offs, sizes, NULL, level, 1, 1, !checksum, SDF_CAP_EXACT, 0, 0, 0, -1, NULL)) return 1;
        if (sdf_batch(9, offs, sizes, pre, level, 1, 1, checksum, SDF_CAP_ONE_BELOW, 0, 0, LZ_FRAME_E(dstMaxSize_tooSmall), -1, NULL)) return 1;
        if (sdf_batch(9, offs, sizes, pre, 23, 1, 1, checksum, SDF_CAP_BOUND, 0, 0, LZ_FRAME_E(compressionLevel_invalid), 0, grown)) return 1;
        CHECK(grown[2] == 0 && grown[3] == 0, "a stream of level 23 launched something");
        if (sdf_batch(4, lateOffs, lateSizes, pre, level, 1, 0, checksum, SDF_CAP_BOUND, 0, 0, LZ_FRAME_E(blockMode_invalid), 2, NULL)) return 1;
        if (sdf_batch(9, offs, sizes, pre, level, 1, 1, checksum, SDF_CAP_BOUND, 1u << 4 | 1u << 7, 0, LZ_FRAME_E(GENERIC), 4, NULL)) return 1;
        /* a refused launch, a failing allocation (fresh stages: one of the first hipMallocs of the call); then a good call */
        sdf_refuse_pack(s & 1 ? 2 : 1);
        if (sdf_batch(6, offs, sizes, pre, level, 1, 1, checksum, SDF_CAP_BOUND, 0, 0, LZ_FRAME_E(GENERIC), -1, NULL)) return 1;
        pf_shutdown();
        if (sdf_batch(6, offs, sizes, pre, level, 1, 1, checksum, SDF_CAP_BOUND, 0, 1 + (int)(s % 3), LZ_FRAME_E(GENERIC), -1, NULL)) return 1;
        if (sdf_batch(6, offs, sizes, pre, level, 1, 1, checksum, SDF_CAP_BOUND, 0, 0, 0, -1, NULL)) return 1;
    }
    unsetenv("LIZARDGPU_FRAME_CHUNK_BLOCKS");
    printf("stream_device_fake: ok, %llu ops\n", fh_ops_run());
    return 0;
}
#endif
