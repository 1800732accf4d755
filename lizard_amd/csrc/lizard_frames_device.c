/* lizard_frames_device.c — LizardGPU_compressFrames_device: many buffers that lie in device memory, one Lizard frame each, in ONE batch
 * (include/lizard_amd.h Part 3).  Plain C on the HIP runtime's C API and the shim of lizard_gpu_ctx.h, like lizard_frame_device.c, whose
 * generalisation from one cursor to one cursor per frame it is.  Per frame it answers what LizardGPU_compressFrame_device answers for
 * that buffer alone: the refusals are lzgpu_frame_device_plan's (lizard_frame_host.c) for both, the header is
 * lzgpu_frame_write_header's, the records are placed by the same rule.
 *
 * Why a batch: a caller with a state_dict or a set of cache pages holds thousands of buffers of a few blocks each.  One call per
 * buffer launches a near-empty device and waits for it, N times, and with a checksum it drags every source through one host thread.
 * Here the blocks of ALL frames form one list in frame order, cut into chunks of at most chunk_blocks blocks as in the sibling (the
 * same LIZARDGPU_FRAME_CHUNK_BLOCKS; the default divides lzp_chunk_bytes by the batch's largest block size).  A chunk may hold many
 * whole frames and a frame may straddle chunks.  Each chunk is one ragged launch of the block kernels into a stage's slots (stream
 * A): block b is blkSizes[b] bytes at base + blkOffsets[b], base being the lowest source address of the batch; the launch's block
 * size is the largest among the chunk's frames.  lz_frames_scan_kernel / lz_frames_gather_kernel (lz_frames_pack.h, stream B) move the
 * records to their frames, whose cursors live in the per-frame table in device memory.  The stages rotate under events exactly as in
 * lizard_frame_device.c (lz_batch_rotate, lizard_device_batch.h: the chunk list is the stream entry's too).  With a checksum
 * lz_xxh32_frames_kernel hashes every source on the device (stream C) beside the compression;
 * lz_frames_finish_kernel (stream B, behind the last gather and the hash) writes headers, end marks and checksums and one result
 * record per frame.  All of it is enqueued before the host waits for anything; the host waits once, for the result records.
 *
 * What crosses PCIe: the two tables going up (88 bytes per frame, 16 per block), 16 bytes per frame coming down.  No payload byte in
 * either direction, checksum or not.
 *
 * One frame's hash is four serial chains, so a batch cannot finish before its largest frame is hashed, at one chain's pace — not
 * measured yet and certainly below a host core's.  A caller with one huge buffer and a checksum belongs with
 * LizardGPU_compressFrame_device. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_batch.h"

typedef struct {
    LzBatch b;                                                /* the blocks of all frames as one list (lizard_device_batch.h) */
    void* const* dsts; const size_t* caps; const void* const* srcs; const size_t* sizes; size_t* results;
    const LizardF_preferences_t* prefsPtr;
    /* the tables of the call: pinned (stage 0's h_aux) and, in the same layout, in device memory (LzCtx::dfTab) behind which the
     * result records follow; those come down into stage 1's h_aux */
    size_t tableBytes;
    LzFramesResult *h_results, *d_results;
} BJob;

static int b_buffers(BJob* j)
{
    LzBatch* b = &j->b;
    LzCtx* c = b->c;
    const size_t F = b->nFrames;
    int rc;
    j->tableBytes = lz_batch_tables_end(b, F * sizeof(LzFramesEntry));
    if ((rc = lzp_ensure_pinned((void**)&c->stage[0].h_aux, &c->stage[0].h_aux_cap, j->tableBytes))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[1].h_aux, &c->stage[1].h_aux_cap, F * sizeof(LzFramesResult)))) return rc;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, j->tableBytes + F * sizeof(LzFramesResult)))) return rc;
    if ((rc = lz_batch_stages(b))) return rc;
    b->h_frames = (LzFramesEntry*)c->stage[0].h_aux;         b->d_frames = (LzFramesEntry*)c->dfTab;
    lz_batch_block_tables(b, c->stage[0].h_aux, c->dfTab, F * sizeof(LzFramesEntry));
    j->h_results = (LzFramesResult*)c->stage[1].h_aux;       j->d_results = (LzFramesResult*)(c->dfTab + j->tableBytes);
    return 0;
}

/* the per-frame and the per-block table, in pinned memory; a refused frame keeps its entry (so that indices stay the caller's) without
 * the LIVE flag, and no blocks */
static void b_tables(BJob* j)
{
    size_t i, at = 0;
    for (i = 0; i < j->b.nFrames; i++) {
        LzFramesEntry* e = &j->b.h_frames[i];
        LizardF_preferences_t prefs;
        size_t bs, nb;
        memset(e, 0, sizeof *e);
        if (j->results[i]) continue;
        (void)lzgpu_frame_device_plan(&prefs, j->prefsPtr, j->dsts[i], j->caps[i], j->srcs[i], j->sizes[i]);
        bs = lzgpu_frame_block_size((unsigned)prefs.frameInfo.blockSizeID);
        nb = (j->sizes[i] + bs - 1) / bs;
        e->dst = (uint64_t)(uintptr_t)j->dsts[i];
        e->limit = (uint64_t)(j->caps[i] - 4 - (size_t)prefs.frameInfo.contentChecksumFlag * 4);      /* (the bound counts both) */
        e->headerBytes = (uint32_t)lzgpu_frame_write_header(e->header, &prefs.frameInfo);
        e->cursor = e->headerBytes;
        e->src = (uint64_t)(uintptr_t)j->srcs[i]; e->srcSize = (uint64_t)j->sizes[i];
        e->blockSize = (uint32_t)bs; e->nBlocks = (uint32_t)nb;
        e->flags = LZK_FRAMES_LIVE | (prefs.frameInfo.contentChecksumFlag == 1 ? LZK_FRAMES_CHECKSUM : 0u);
        lz_batch_blocks(&j->b, &at, i, j->srcs[i], j->sizes[i], bs, nb);
    }
}

/* a chunk's records move to their frames (lz_batch_rotate's pack) */
static int b_pack(void* arg, const LzBatch* b, const LzStage* s, size_t first, size_t q, size_t bs, uint32_t* d_sizes, uint64_t* d_offsets)
{
    (void)arg;
    return lzk_frames_pack_launch(b->base, b->d_blkOffsets + first, b->d_blkSizes + first, b->d_blkFrames + first, s->d_slots, lz_bound_slot(bs), d_sizes,
                                  d_offsets, (uint32_t)q, b->d_frames, b->B);
}

/* every chunk, the hash, the finish and the copy of the result records: enqueued, nothing waited for */
static int b_enqueue(BJob* j)
{
    LzBatch* b = &j->b;
    LzCtx* c = b->c;
    int rc;
    if ((rc = lz_batch_rotate(b, b_pack, NULL, &c->devFrameCompressStats[2], NULL))) return rc;
    if ((rc = lzk_frames_finish_launch(b->d_frames, j->d_results, (uint32_t)b->nFrames, b->B))) return rc;
    LZ_HIP(hipMemcpyAsync(j->h_results, j->d_results, b->nFrames * sizeof(LzFramesResult), hipMemcpyDeviceToHost, b->B));
    LZ_HIP(hipEventRecord(c->stage[0].meta, b->B));
    return 0;
}

/* the only wait of the call; then every live frame's answer */
static int b_collect(BJob* j)
{
    LzCtx* c = j->b.c;
    size_t i;
    LZ_HIP(hipEventSynchronize(c->stage[0].meta));
    for (i = 0; i < j->b.nFrames; i++) {
        const LzFramesResult* r = &j->h_results[i];
        if (j->results[i]) continue;
        if (r->size == LZK_FRAMES_OVERFLOW) { j->results[i] = LZ_FRAME_E(dstMaxSize_tooSmall); continue; }
        j->results[i] = (size_t)r->size;
        c->devFrameCompressStats[0] += (unsigned long long)j->b.h_frames[i].nBlocks - r->rawRecords;
        c->devFrameCompressStats[1] += r->rawRecords;
    }
    return 0;
}

static void b_first_refusal(size_t nFrames, const size_t* results)      /* the error text of a call that did its work: the first frame that was refused */
{
    size_t i;
    for (i = 0; i < nFrames; i++)
        if (LizardGPU_frameIsError(results[i])) {
            snprintf(lzk_err(), LZK_ERR_BYTES, "frame %zu refused: %s", i, results[i] == LZ_FRAME_E(GENERIC) ? "bad argument (null pointer)" : LizardF_getErrorName(results[i]));
            return;
        }
}

int LizardGPU_compressFrames_device(size_t nFrames, void* const* d_dsts, const size_t* dstCapacities, const void* const* d_srcs,
                                    const size_t* srcSizes, size_t* results, const LizardGPU_framePrefs_t* preferencesPtr, void* stream)
{
    LizardF_preferences_t prefs;
    BJob j;
    LzGuard g;
    size_t i, live = 0;
    int rc;
    lzk_err()[0] = 0;
    if (!nFrames) return 0;
    if (!d_dsts || !dstCapacities || !d_srcs || !srcSizes || !results || nFrames > 0x7FFFFFFFu) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null array or more than 2^31 - 1 frames)");
        return -LIZARDGPU_ERR_ARG;
    }
    memset(&j, 0, sizeof j);
    j.b.nFrames = nFrames; j.dsts = d_dsts; j.caps = dstCapacities; j.srcs = d_srcs; j.sizes = srcSizes; j.results = results; j.prefsPtr = preferencesPtr;
    /* every frame's refusal, before anything is enqueued; results[i] stays 0 for the frames that go on */
    for (i = 0; i < nFrames; i++) {
        results[i] = lzgpu_frame_device_plan(&prefs, preferencesPtr, d_dsts[i], dstCapacities[i], d_srcs[i], srcSizes[i]);
        if (results[i]) continue;
        {
            const size_t bs = lzgpu_frame_block_size((unsigned)prefs.frameInfo.blockSizeID), nb = (srcSizes[i] + bs - 1) / bs;
            live++;
            j.b.hash = prefs.frameInfo.contentChecksumFlag == 1;
            j.b.level = lzk_clamp_level(prefs.compressionLevel);
            if (!nb) continue;
            j.b.nBlocks += nb;
            if (bs > j.b.maxBlock) j.b.maxBlock = bs;
            if (!j.b.base || (const uint8_t*)d_srcs[i] < j.b.base) j.b.base = (const uint8_t*)d_srcs[i];
        }
    }
    if (!live) { b_first_refusal(nFrames, results); return 0; }
    if (j.b.nBlocks > 0xFFFFFFFFu) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (more than 2^32 - 1 blocks in one batch)");
        for (i = 0; i < nFrames; i++) if (!results[i]) results[i] = LZ_FRAME_E(GENERIC);
        return -LIZARDGPU_ERR_ARG;
    }
    lzk_guard_acquire(&g);
    rc = g.rc;
    if (!rc) {
        j.b.c = g.c;
        rc = lzk_ctx_init(g.c);
        if (!rc) {
            j.b.perChunk = lz_frame_chunk_blocks(g.c, j.b.maxBlock ? j.b.maxBlock : lzgpu_frame_block_size(1));
            j.b.nChunks = (j.b.nBlocks + j.b.perChunk - 1) / j.b.perChunk;
            rc = b_buffers(&j);
        }
        if (!rc) {
            b_tables(&j);
            g.c->hostKernelMs = -1.0f;
            rc = lz_batch_upload(&j.b, j.b.d_frames, j.b.h_frames, j.tableBytes, (hipStream_t)stream);
        }
        if (!rc) rc = b_enqueue(&j);
        if (!rc) rc = b_collect(&j);
        lz_quiesce(g.c);
        lzk_guard_release(&g);
    }
    if (rc) {
        for (i = 0; i < nFrames; i++) if (!results[i] || !LizardGPU_frameIsError(results[i])) results[i] = LZ_FRAME_E(GENERIC);
        return rc;
    }
    b_first_refusal(nFrames, results);
    return 0;
}
