/* lizard_seek_device.c — seekable streams in device memory (include/lizard_amd.h Part 3b): LizardGPU_compressSeekableStream_device writes
 * a stream with the seek table of lizard_seek_host.c behind its last frame; LizardGPU_seekTable_device reads that table back;
 * LizardGPU_decompressSeekableStream_device decodes the stream without the serial walk and LizardGPU_decompressStreamItems_device only
 * the items a caller lists.  Plain C on the HIP runtime's C API.
 *
 * This file adds no machinery of its own.  The writer is lzgpu_stream_compress (lizard_stream_device.c) with the table's bytes as its
 * extra fixed bytes and one launch (lz_stream_seektable_kernel, lz_stream_pack.h) as its hook behind the finish kernel: still one wait.
 * The readers are the table — two small copies from the end of the stream — and ONE call of LizardGPU_decompressFrames_device with
 * the places the table names.  The table LOCATES and never decides an answer: whatever the batch does not answer exactly as the
 * table says sends the whole-stream reader back to LizardGPU_decompressStream_device from the start, whose answer is returned, so
 * identity with that entry holds by construction and no order of refusals is derived twice. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_common.h"

#define SK_FOOTER 16u
#define SK_MIN    48u                                         /* the table frame of one item */

/* ---- writer ---- */

static int k_table_hook(void* arg, const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const LzStreamState* d_state,
                        const uint64_t* d_offsets, uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, hipStream_t B)
{
    (void)arg;
    return lzk_stream_seektable_launch(d_frames, d_entries, d_state, d_offsets, nFrames, fixedTotal, capacity, B);
}

size_t LizardGPU_compressSeekableStream_device(void* d_dst, size_t dstCapacity, size_t nFrames, const void* const* d_srcs, const size_t* srcSizes,
                                               const void* const* prefixes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs,
                                               uint64_t* frameOffsets, size_t* failedFrame, void* stream)
{
    const size_t tableBytes = LizardGPU_seekTableBytes(nFrames);
    size_t i, r;
    if (!nFrames) return 0;
    lzk_err()[0] = 0;
    if (LizardGPU_frameIsError(tableBytes)) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (the seek table of %zu items does not fit its size field)", nFrames);
        return LZ_FRAME_E(GENERIC);
    }
    for (i = 0; prefixSizes && i < nFrames; i++)
        if ((uint64_t)prefixSizes[i] > 0xFFFFFFFFull) {
            if (failedFrame) *failedFrame = i;
            snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (frame %zu: a prefix of 2^32 bytes or more does not fit a seek table entry)", i);
            return LZ_FRAME_E(GENERIC);
        }
    r = lzgpu_stream_compress(d_dst, dstCapacity, nFrames, d_srcs, srcSizes, prefixes, prefixSizes, prefs, frameOffsets, failedFrame, stream,
                              (uint64_t)tableBytes, k_table_hook, NULL);
    if (!LizardGPU_frameIsError(r) && frameOffsets) frameOffsets[nFrames] -= (uint64_t)tableBytes;      /* where the table starts */
    return r;
}

/* ---- the table, out of device memory ---- */

static void k_stats_add(unsigned which, unsigned long long add)       /* the error text survives */
{
    char keep[LZK_ERR_BYTES];
    LzCtx* c;
    lz_err_save(keep);
    if ((c = lzk_ctx_peek())) {
        pthread_mutex_lock(&c->mu);
        c->devSeekStats[which] += add;
        pthread_mutex_unlock(&c->mu);
    }
    lz_err_restore(keep);
}

/* `bytes` from d_src into the pinned buffer of stage 1, behind what the caller's stream holds: one copy, one wait */
static int k_copy_down(LzCtx* c, const void* d_src, size_t bytes, hipStream_t stream)
{
    int rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[1].h_aux, &c->stage[1].h_aux_cap, bytes))) return rc;
    LZ_HIP(hipMemcpyAsync(c->stage[1].h_aux, d_src, bytes, hipMemcpyDeviceToHost, stream));
    LZ_HIP(hipStreamSynchronize(stream));
    return 0;
}

/* LIZARDGPU_SEEK_USABLE with *entries (malloc'd, the caller frees: *n of them), LIZARDGPU_SEEK_NONE / _DAMAGED, or -LIZARDGPU_ERR_* */
static int k_load(const void* d_src, size_t srcSize, LizardGPU_seekEntry_t** entries, size_t* n, uint64_t* tableOffset, hipStream_t stream)
{
    const uint8_t* const src = (const uint8_t*)d_src;
    LzGuard g;
    size_t bytes;
    int rc;
    *entries = NULL; *n = 0; *tableOffset = 0;
    if (srcSize < SK_MIN) return LIZARDGPU_SEEK_NONE;
    lzk_guard_acquire(&g);                                     /* the context's pinned buffer is ours, its device current, until the table is parsed */
    if (g.rc) return g.rc;
    rc = lzk_ctx_init(g.c);
    if (!rc) rc = k_copy_down(g.c, src + srcSize - SK_FOOTER, SK_FOOTER, stream);
    if (!rc) rc = LizardGPU_seekTableRead(g.c->stage[1].h_aux, SK_FOOTER, (uint64_t)srcSize, NULL, 0, n, tableOffset);
    if (rc == LIZARDGPU_SEEK_MORE) {
        bytes = LizardGPU_seekTableBytes(*n);                  /* (<= srcSize: the codec said so) */
        *entries = (LizardGPU_seekEntry_t*)malloc(*n * sizeof **entries);
        if (!*entries) { snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); rc = -LIZARDGPU_ERR_NOMEM; }
        else rc = k_copy_down(g.c, src + srcSize - bytes, bytes, stream);
        if (!rc) rc = LizardGPU_seekTableRead(g.c->stage[1].h_aux, bytes, (uint64_t)srcSize, *entries, *n, n, tableOffset);
        if (rc == LIZARDGPU_SEEK_MORE) rc = LIZARDGPU_SEEK_DAMAGED;                 /* (cannot be: the tail is what the codec asked for) */
    }
    lzk_guard_release(&g);
    if (rc != LIZARDGPU_SEEK_USABLE) { free(*entries); *entries = NULL; }
    else k_stats_add(3, 1);
    return rc;
}

int LizardGPU_seekTable_device(const void* d_src, size_t srcSize, LizardGPU_seekEntry_t* entries, size_t maxEntries, size_t* n, uint64_t* tableOffset,
                               void* stream)
{
    LizardGPU_seekEntry_t* e = NULL;
    int rc;
    lzk_err()[0] = 0;
    if (n) *n = 0;
    if (tableOffset) *tableOffset = 0;
    if (!d_src || !n || !tableOffset || (maxEntries && !entries)) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null pointer)"); return -LIZARDGPU_ERR_ARG; }
    rc = k_load(d_src, srcSize, &e, n, tableOffset, (hipStream_t)stream);
    if (rc == LIZARDGPU_SEEK_USABLE && maxEntries) memcpy(entries, e, (*n < maxEntries ? *n : maxEntries) * sizeof *e);
    free(e);
    return rc;
}

/* ---- readers ---- */

/* the host arrays of one batch, in one allocation */
typedef struct { void** dsts; const void** srcs; size_t *caps, *sizes, *results, *used; } KBatch;
static int k_batch(KBatch* b, size_t n)
{
    b->dsts = (void**)malloc(n * (2 * sizeof(void*) + 4 * sizeof(size_t)));
    if (!b->dsts) { snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); return -LIZARDGPU_ERR_NOMEM; }
    b->srcs = (const void**)(b->dsts + n);
    b->caps = (size_t*)(b->srcs + n); b->sizes = b->caps + n; b->results = b->sizes + n; b->used = b->results + n;
    return 0;
}

/* the whole stream through the table: 1 with *sum and *frames when every frame answered exactly its entry, else 0 */
static int k_fast(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* sum, size_t* frames, unsigned flags, void* stream)
{
    LizardGPU_seekEntry_t* e = NULL;
    KBatch b = { 0 };
    size_t n = 0, i, m = 0, place = 0;
    uint64_t tableOffset = 0, total = 0;
    int good = 0;
    if (k_load(d_src, srcSize, &e, &n, &tableOffset, (hipStream_t)stream) != LIZARDGPU_SEEK_USABLE) return 0;
    for (i = 0; i < n; i++) total += e[i].decodedBytes;       /* (does not wrap: the table is usable) */
    if (total <= (uint64_t)dstCapacity && !k_batch(&b, 2 * n)) {        /* (n < 2^28: the size field holds the table) */
        for (i = 0; i < n; i++) {
            const uint64_t end = i + 1 < n ? e[i + 1].offset : tableOffset;
            uint8_t* const at = d_dst ? (uint8_t*)d_dst + place : NULL;
            if (e[i].prefixBytes) {
                b.srcs[m] = (const uint8_t*)d_src + e[i].offset; b.sizes[m] = e[i].prefixBytes; b.dsts[m] = at; b.caps[m] = 0;
                m++;
            }
            b.srcs[m] = (const uint8_t*)d_src + e[i].offset + e[i].prefixBytes; b.sizes[m] = (size_t)(end - e[i].offset - e[i].prefixBytes);
            b.dsts[m] = at; b.caps[m] = (size_t)e[i].decodedBytes;
            m++;
            place += (size_t)e[i].decodedBytes;
        }
        if (!LizardGPU_decompressFrames_device(m, b.dsts, b.caps, b.srcs, b.sizes, b.results, b.used, flags, stream)) {
            for (i = 0; i < m && b.results[i] == b.caps[i] && b.used[i] == b.sizes[i]; i++) { }
            good = i == m;
        }
    }
    free(b.dsts);
    free(e);
    *sum = (size_t)total; *frames = m + 1;                     /* (+ the table frame) */
    return good;
}

size_t LizardGPU_decompressSeekableStream_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr,
                                                 size_t* nFramesPtr, size_t* decodedPtr, unsigned flags, void* stream)
{
    size_t sum = 0, frames = 0;
    if (!srcSize) return 0;
    if (d_src && (d_dst || !dstCapacity) && k_fast(d_dst, dstCapacity, d_src, srcSize, &sum, &frames, flags, stream)) {
        k_stats_add(0, 1);
        if (srcConsumedPtr) *srcConsumedPtr = srcSize;
        if (nFramesPtr) *nFramesPtr = frames;
        if (decodedPtr) *decodedPtr = sum;
        lzk_err()[0] = 0;
        return sum;
    }
    k_stats_add(1, 1);
    return LizardGPU_decompressStream_device(d_dst, dstCapacity, d_src, srcSize, srcConsumedPtr, nFramesPtr, decodedPtr, flags, stream);
}

size_t LizardGPU_decompressStreamItems_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, const size_t* items, size_t nItems,
                                              uint64_t* itemOffsets, size_t* failedItem, unsigned flags, void* stream)
{
    LizardGPU_seekEntry_t* e = NULL;
    KBatch b = { 0 };
    size_t n = 0, k, answer;
    uint64_t tableOffset = 0, total = 0;
    int rc;
    if (!nItems) return 0;
    lzk_err()[0] = 0;
    if (!d_src || !items || (!d_dst && dstCapacity)) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null pointer)"); return LZ_FRAME_E(GENERIC); }
    rc = k_load(d_src, srcSize, &e, &n, &tableOffset, (hipStream_t)stream);
    if (rc < 0) { if (!lzk_err()[0]) snprintf(lzk_err(), LZK_ERR_BYTES, "reading the seek table failed (LIZARDGPU_ERR %d)", -rc); return LZ_FRAME_E(GENERIC); }
    if (rc != LIZARDGPU_SEEK_USABLE) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "the stream has no usable seek table (%s)", rc == LIZARDGPU_SEEK_NONE ? "none at its end" : "damaged");
        return LZ_FRAME_E(frameType_unknown);
    }
    answer = 0;
    for (k = 0; k < nItems && !answer; k++) {
        if (items[k] >= n) {
            snprintf(lzk_err(), LZK_ERR_BYTES, "items[%zu] = %zu, the stream has %zu items", k, items[k], n);
            answer = LZ_FRAME_E(frameSize_wrong);
        } else if (k && items[k] <= items[k - 1]) {
            snprintf(lzk_err(), LZK_ERR_BYTES, "items[%zu] = %zu does not ascend from items[%zu] = %zu", k, items[k], k - 1, items[k - 1]);
            answer = LZ_FRAME_E(blockMode_invalid);
        } else total += e[items[k]].decodedBytes;
        if (answer && failedItem) *failedItem = k;
    }
    if (!answer && total > (uint64_t)dstCapacity) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "the listed items decode to %llu bytes, dstCapacity = %zu", (unsigned long long)total, dstCapacity);
        answer = LZ_FRAME_E(dstMaxSize_tooSmall);
    }
    if (!answer && k_batch(&b, nItems)) answer = LZ_FRAME_E(GENERIC);
    if (!answer) {
        size_t place = 0;
        for (k = 0; k < nItems; k++) {
            const LizardGPU_seekEntry_t* const x = &e[items[k]];
            const uint64_t end = items[k] + 1 < n ? x[1].offset : tableOffset;
            b.srcs[k] = (const uint8_t*)d_src + x->offset + x->prefixBytes; b.sizes[k] = (size_t)(end - x->offset - x->prefixBytes);
            b.dsts[k] = d_dst ? (uint8_t*)d_dst + place : NULL; b.caps[k] = (size_t)x->decodedBytes;
            if (itemOffsets) itemOffsets[k] = (uint64_t)place;
            place += (size_t)x->decodedBytes;
        }
        if (itemOffsets) itemOffsets[nItems] = (uint64_t)place;
        rc = LizardGPU_decompressFrames_device(nItems, b.dsts, b.caps, b.srcs, b.sizes, b.results, b.used, flags, stream);
        if (rc) {
            if (!lzk_err()[0]) snprintf(lzk_err(), LZK_ERR_BYTES, "the batch decoder failed (LIZARDGPU_ERR %d)", -rc);
            answer = LZ_FRAME_E(GENERIC);
        }
        for (k = 0; k < nItems && !answer; k++) {
            if (b.results[k] == b.caps[k] && b.used[k] == b.sizes[k]) continue;
            answer = LizardGPU_frameIsError(b.results[k]) ? b.results[k] : LZ_FRAME_E(decompressionFailed);
            if (failedItem) *failedItem = k;
            snprintf(lzk_err(), LZK_ERR_BYTES, "item %zu (items[%zu]) at offset %llu does not answer its seek table entry: %s", items[k], k,
                     (unsigned long long)e[items[k]].offset,
                     LizardGPU_frameIsError(b.results[k]) ? LizardF_getErrorName(b.results[k]) : "another size, or bytes left in its region");
        }
        if (!answer) { answer = place; k_stats_add(2, nItems); lzk_err()[0] = 0; }
    }
    free(b.dsts);
    free(e);
    return answer;
}

int LizardGPU_seekDeviceStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devSeekStats));
}
