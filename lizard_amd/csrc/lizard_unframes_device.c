/* lizard_unframes_device.c — LizardGPU_decompressFrames_device / LizardGPU_framesInfo_device: many frames that lie in device memory,
 * each decoded into its own device buffer, in ONE batch (include/lizard_amd.h Part 3b).  Plain C on the HIP runtime's C API and the
 * shim of lizard_gpu_ctx.h, like lizard_unframe_device.c, whose answer it reproduces frame by frame, and the reading half of
 * lizard_frames_device.c.
 *
 * Why a batch: the single-frame entry takes the context, walks, decodes and waits at least three times per frame, and its decode
 * launch holds one frame's records where the device has room for thousands; with a checksum every decoded byte crosses PCIe to be
 * hashed by the calling thread.  Here the host waits twice per CALL:
 *   count pass   one table entry per frame goes up; lz_unframes_walk_kernel (unframes_kernels.h) walks every frame, one wave each, side
 *                by side, without tables; one LzWalkResult per frame comes down (what an entry that is not walked has there is
 *                never looked at).  The host answers what is decided now — a chain the walk refuses is -(status), a skippable frame
 *                is 0 bytes — and gives every other frame its first index in ONE record list (a prefix sum of the record counts).
 *   fill pass    the same walk again, writing every frame's payload offsets and record words at its base in the batch tables; ONE
 *                decode launch over all records of all frames, each in place in its frame's buffer (lz_unframes_kernel); the settle
 *                kernel (clean or not, decoded size); lz_xxh32_frames_kernel over a table whose sources are the DECODED frames and
 *                whose lengths the settle kernel wrote, for the frames that carry a checksum the caller wants verified; the finish
 *                kernel (content size, stored checksum); one copy of the result records.  All enqueued on one stream without a wait.
 * No staging slots, no chunking: the tables cost 20 bytes per record and 240 per frame.  No payload byte crosses PCIe, checksum or not.
 *
 * The device settles only CLEAN frames: every record decoded, every record but the last filled the frame's block size, the size is
 * the header's content size when there is one, the checksum matches when verified — every frame LizardGPU_compressFrames_device
 * writes, decoded into room enough.  Every other frame the walk accepted (a short record in the middle, a record that failed or
 * needs its history, a slot at or behind the capacity, a wrong size or checksum) is handed to LizardGPU_decompressFrame_device with
 * the same arguments after the batch part, one by one: identity with that entry holds by construction there, and this file never
 * re-derives the order of its refusals.  LizardGPU_framesDecodeDeviceStats counts them. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_batch.h"

enum { U_OPEN = 0, U_DECIDED = 1, U_DELEGATE = 2 };           /* a frame's state on the host */

typedef struct {
    LzCtx* c;
    size_t nFrames, nRecords;
    void* const* dsts; const size_t* caps; const void* const* srcs; const size_t* sizes;
    unsigned flags;
    unsigned char* state;                                     /* U_*, one per frame */
    /* what goes up, in pinned memory (stage 0's h_aux) and in the same layout at the head of LzCtx::dfTab: the frame table, the
     * table the hash kernel works from, the frame of every record; behind them in dfTab only: walk results, result records (both
     * come down into stage 1's h_aux), payload offsets, record words, per-record results */
    size_t upBytes;
    LzUnframesEntry *h_frames, *d_frames;
    LzFramesEntry *h_hash, *d_hash;
    uint32_t *h_recFrame, *d_recFrame;
    LzWalkResult *h_walk, *d_walk;
    LzUnframesResult *h_results, *d_results;
    uint64_t* d_offs; uint32_t *d_words, *d_out;
    hipStream_t S;
} UJob;

/* the tables for nFrames frames and R records (the count pass has R = 0: the frame table alone goes up) */
static int u_buffers(UJob* j, size_t R)
{
    LzCtx* c = j->c;
    const size_t F = j->nFrames;
    const size_t oHash = F * sizeof(LzUnframesEntry), oRecFrame = oHash + F * sizeof(LzFramesEntry);
    const size_t oWalk = (oRecFrame + 4 * R + 7) & ~(size_t)7, oRes = oWalk + F * sizeof(LzWalkResult);
    const size_t oOffs = oRes + F * sizeof(LzUnframesResult), oWords = oOffs + 8 * R, oOut = oWords + 4 * R;
    int rc;
    j->upBytes = oWalk;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[0].h_aux, &c->stage[0].h_aux_cap, j->upBytes))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[1].h_aux, &c->stage[1].h_aux_cap, F * (sizeof(LzWalkResult) + sizeof(LzUnframesResult))))) return rc;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, oOut + 4 * R))) return rc;
    j->h_frames = (LzUnframesEntry*)c->stage[0].h_aux;          j->d_frames = (LzUnframesEntry*)c->dfTab;
    j->h_hash = (LzFramesEntry*)(c->stage[0].h_aux + oHash);    j->d_hash = (LzFramesEntry*)(c->dfTab + oHash);
    j->h_recFrame = (uint32_t*)(c->stage[0].h_aux + oRecFrame); j->d_recFrame = (uint32_t*)(c->dfTab + oRecFrame);
    j->h_walk = (LzWalkResult*)c->stage[1].h_aux;               j->d_walk = (LzWalkResult*)(c->dfTab + oWalk);
    j->h_results = (LzUnframesResult*)(c->stage[1].h_aux + F * sizeof(LzWalkResult)); j->d_results = (LzUnframesResult*)(c->dfTab + oRes);
    j->d_offs = (uint64_t*)(c->dfTab + oOffs); j->d_words = (uint32_t*)(c->dfTab + oWords); j->d_out = (uint32_t*)(c->dfTab + oOut);
    j->S = c->stage[1].stream;
    return 0;
}

/* the count pass over every frame the host has not answered: the first wait */
static int u_count_pass(UJob* j, hipStream_t stream)
{
    return lz_count_pass(j->c, j->nFrames, j->state, j->srcs, sizeof j->srcs[0], j->sizes, sizeof j->sizes[0], j->h_frames, j->d_frames, j->h_walk,
                         j->d_walk, j->S, stream);
}

/* the tables of the fill pass, from the caller's arrays and the walk results (the pinned table may have moved since the count pass) */
static void u_fill_tables(UJob* j)
{
    size_t i, first = 0, k;
    for (i = 0; i < j->nFrames; i++) {
        LzUnframesEntry* e = &j->h_frames[i];
        LzFramesEntry* h = &j->h_hash[i];
        const LzWalkResult* w = &j->h_walk[i];
        memset(e, 0, sizeof *e);
        memset(h, 0, sizeof *h);
        if (j->state[i] != U_OPEN) continue;
        lz_fill_entry(e, j->srcs[i], j->sizes[i], first, w);
        e->dst = (uint64_t)(uintptr_t)j->dsts[i]; e->cap = (uint64_t)j->caps[i];
        if (w->checksumFlag && !(j->flags & LIZARDGPU_FRAME_SKIP_CHECKSUM)) e->flags |= LZU_VERIFY;
        h->src = e->dst;                                        /* srcSize: the settle kernel's to write */
        if (e->flags & LZU_VERIFY) h->flags = LZK_FRAMES_LIVE | LZK_FRAMES_CHECKSUM;
        for (k = 0; k < (size_t)w->nRecords; k++) j->h_recFrame[first + k] = (uint32_t)i;
        first += (size_t)w->nRecords;
    }
}

/* everything behind the count pass, enqueued without a wait in between; then the second wait */
static int u_fill_pass(UJob* j, int anyHash)
{
    LzCtx* c = j->c;
    const uint32_t F = (uint32_t)j->nFrames;
    int rc;
    LZ_HIP(hipMemcpyAsync(j->d_frames, j->h_frames, j->upBytes, hipMemcpyHostToDevice, j->S));
    if (j->nRecords) {
        if ((rc = lzk_unframes_walk_launch(j->d_frames, F, 1, j->d_offs, j->d_words, j->d_walk, j->S))) return rc;
        if ((rc = lzk_unframes_decode_launch(c, j->d_frames, j->d_offs, j->d_words, j->d_recFrame, j->d_out, j->nRecords, j->S))) return rc;
    }
    if ((rc = lzk_unframes_settle_launch(j->d_frames, F, j->d_out, j->d_results, j->d_hash, j->S))) return rc;
    if (anyHash && (rc = lzk_frames_hash_launch(j->d_hash, F, j->S))) return rc;
    if ((rc = lzk_unframes_finish_launch(j->d_frames, F, j->d_hash, j->d_results, j->S))) return rc;
    LZ_HIP(hipMemcpyAsync(j->h_results, j->d_results, j->nFrames * sizeof(LzUnframesResult), hipMemcpyDeviceToHost, j->S));
    LZ_HIP(hipEventRecord(c->stage[0].meta, j->S));
    LZ_HIP(hipEventSynchronize(c->stage[0].meta));
    return 0;
}

/* The batch part under the context guard.  0, or -LIZARDGPU_ERR_*; on 0 every frame is U_DECIDED (answered) or U_DELEGATE. */
static int u_batch(UJob* j, size_t* results, size_t* consumed, hipStream_t stream)
{
    LzCtx* c = j->c;
    size_t i, open = 0;
    int rc, anyHash = 0;
    if ((rc = lzk_ctx_init(c))) return rc;
    if ((rc = u_buffers(j, 0))) return rc;
    c->hostKernelMs = -1.0f;
    if ((rc = u_count_pass(j, stream))) return rc;
    c->devFramesDecodeStats[3]++;
    for (i = 0; i < j->nFrames; i++) {
        const LzWalkResult* w = &j->h_walk[i];
        if (j->state[i] != U_OPEN) continue;
        if (w->status) { results[i] = (size_t)-(long)w->status; j->state[i] = U_DECIDED; }
        else if (w->frameType) { results[i] = 0; if (consumed) consumed[i] = (size_t)w->frameBytes; j->state[i] = U_DECIDED; }
        else {
            if (w->nRecords > 0xFFFFFFFFull || j->nRecords + (size_t)w->nRecords > 0xFFFFFFFFull) {
                snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (2^32 or more block records in one batch)");
                return -LIZARDGPU_ERR_ARG;
            }
            j->nRecords += (size_t)w->nRecords;
            anyHash |= w->checksumFlag && !(j->flags & LIZARDGPU_FRAME_SKIP_CHECKSUM);
            open++;
        }
    }
    if (!open) return 0;
    if ((rc = u_buffers(j, j->nRecords))) return rc;
    u_fill_tables(j);
    if ((rc = u_fill_pass(j, anyHash))) return rc;
    for (i = 0; i < j->nFrames; i++) {
        const LzUnframesResult* r = &j->h_results[i];
        if (j->state[i] != U_OPEN) continue;
        if (r->state == LZU_CLEAN) {
            results[i] = (size_t)r->size; if (consumed) consumed[i] = (size_t)j->h_walk[i].frameBytes;
            j->state[i] = U_DECIDED;
            c->devFramesDecodeStats[1]++;
        } else {
            j->state[i] = U_DELEGATE;
            c->devFramesDecodeStats[2]++;
        }
    }
    c->devFramesDecodeStats[0] += j->nRecords;
    return 0;
}

int LizardGPU_decompressFrames_device(size_t nFrames, void* const* d_dsts, const size_t* dstCapacities, const void* const* d_srcs,
                                      const size_t* srcSizes, size_t* results, size_t* srcConsumed, unsigned flags, void* stream)
{
    UJob j;
    LzGuard g;
    size_t i, open = 0;
    int rc;
    lzk_err()[0] = 0;
    if (!nFrames) return 0;
    if (!d_dsts || !dstCapacities || !d_srcs || !srcSizes || !results || nFrames > 0xFFFFFFFFull) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null array or 2^32 or more frames)");
        return -LIZARDGPU_ERR_ARG;
    }
    memset(&j, 0, sizeof j);
    j.nFrames = nFrames; j.dsts = d_dsts; j.caps = dstCapacities; j.srcs = d_srcs; j.sizes = srcSizes; j.flags = flags;
    if (!(j.state = (unsigned char*)calloc(nFrames, 1))) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory");
        for (i = 0; i < nFrames; i++) { results[i] = LZ_FRAME_E(GENERIC); if (srcConsumed) srcConsumed[i] = 0; }
        return -LIZARDGPU_ERR_NOMEM;
    }
    for (i = 0; i < nFrames; i++) {
        results[i] = 0;
        if (srcConsumed) srcConsumed[i] = 0;
        if ((!d_dsts[i] && dstCapacities[i]) || (!d_srcs[i] && srcSizes[i])) { results[i] = LZ_FRAME_E(GENERIC); j.state[i] = U_DECIDED; }
        else open++;
    }
    rc = 0;
    if (open) {
        lzk_guard_acquire(&g);
        rc = g.rc;
        if (!rc) {
            j.c = g.c;
            rc = u_batch(&j, results, srcConsumed, (hipStream_t)stream);
            lz_quiesce(g.c);
            lzk_guard_release(&g);                             /* (the single-frame entry takes it itself) */
        }
    }
    if (rc) {
        char keep[LZK_ERR_BYTES];
        lz_err_save(keep);
        for (i = 0; i < nFrames; i++) if (j.state[i] != U_DECIDED) { results[i] = LZ_FRAME_E(GENERIC); if (srcConsumed) srcConsumed[i] = 0; }
        free(j.state);
        lz_err_restore(keep);
        return rc;
    }
    for (i = 0; i < nFrames; i++) {
        size_t used = 0;
        if (j.state[i] != U_DELEGATE) continue;
        results[i] = LizardGPU_decompressFrame_device(d_dsts[i], dstCapacities[i], d_srcs[i], srcSizes[i], &used, flags, stream);
        if (srcConsumed) srcConsumed[i] = used;
    }
    free(j.state);
    lz_first_refusal(nFrames, results);
    return 0;
}

int LizardGPU_framesInfo_device(size_t nFrames, const void* const* d_srcs, const size_t* srcSizes, LizardGPU_frameInfo_t* infos,
                                size_t* nRecords, size_t* frameBytes, int* codes, void* stream)
{
    UJob j;
    LzGuard g;
    size_t i, open = 0;
    int rc = 0;
    lzk_err()[0] = 0;
    if (!nFrames) return 0;
    if (!d_srcs || !srcSizes || nFrames > 0xFFFFFFFFull) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null array or 2^32 or more frames)");
        return -LIZARDGPU_ERR_ARG;
    }
    memset(&j, 0, sizeof j);
    j.nFrames = nFrames; j.srcs = d_srcs; j.sizes = srcSizes;
    if (!(j.state = (unsigned char*)calloc(nFrames, 1))) { snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); return -LIZARDGPU_ERR_NOMEM; }
    for (i = 0; i < nFrames; i++) {
        if (nRecords) nRecords[i] = 0;
        if (frameBytes) frameBytes[i] = 0;
        if (codes) codes[i] = 0;
        if (!d_srcs[i] && srcSizes[i]) { if (codes) codes[i] = -(int)LIZARDGPU_FRAME_ERR_GENERIC; j.state[i] = U_DECIDED; }
        else open++;
    }
    if (open) {
        lzk_guard_acquire(&g);
        rc = g.rc;
        if (!rc) {
            j.c = g.c;
            rc = lzk_ctx_init(g.c);
            if (!rc) rc = u_buffers(&j, 0);
            if (!rc) rc = u_count_pass(&j, (hipStream_t)stream);
            for (i = 0; i < nFrames && !rc; i++) {
                const LzWalkResult* w = &j.h_walk[i];
                if (j.state[i] != U_OPEN) continue;
                if (infos && w->infoValid) lz_walk_info(&infos[i], w);
                if (w->status) { if (codes) codes[i] = -(int)w->status; continue; }
                if (nRecords) nRecords[i] = (size_t)w->nRecords;
                if (frameBytes) frameBytes[i] = (size_t)w->frameBytes;
            }
            lz_quiesce(g.c);
            lzk_guard_release(&g);
        }
    }
    if (rc) for (i = 0; i < nFrames; i++) if (codes) codes[i] = -(int)LIZARDGPU_FRAME_ERR_GENERIC;
    free(j.state);
    return rc;
}

int LizardGPU_framesDecodeDeviceStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devFramesDecodeStats));
}
