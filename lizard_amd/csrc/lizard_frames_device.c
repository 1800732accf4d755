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
 * lizard_frame_device.c.  With a checksum lz_xxh32_frames_kernel hashes every source on the device (stream C) beside the compression;
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
#include "lizard_device_common.h"

/* a stage's device tables (its d_aux): the compressed sizes and the record positions of the chunk it holds */
static size_t b_aux_bytes(size_t P) { return ((4 * P + 7) & ~(size_t)7) + 8 * P; }

typedef struct {
    LzCtx* c;
    size_t nFrames, nBlocks, maxBlock, perChunk, nChunks;
    void* const* dsts; const size_t* caps; const void* const* srcs; const size_t* sizes; size_t* results;
    const LizardF_preferences_t* prefsPtr;
    const uint8_t* base;                                      /* the lowest source address among the frames that have blocks */
    int level, hash;
    /* the tables of the call: pinned (stage 0's h_aux) and, in the same layout, in device memory (LzCtx::dfTab) behind which the
     * result records follow; those come down into stage 1's h_aux */
    size_t tableBytes;
    LzFramesEntry *h_frames, *d_frames;
    uint64_t *h_blkOffsets, *d_blkOffsets;
    uint32_t *h_blkSizes, *d_blkSizes, *h_blkFrames, *d_blkFrames;
    LzFramesResult *h_results, *d_results;
    hipStream_t A, B, C;
} BJob;

static int b_buffers(BJob* j)
{
    LzCtx* c = j->c;
    const size_t F = j->nFrames, T = j->nBlocks, P = T < j->perChunk ? T : j->perChunk;
    const size_t oOff = F * sizeof(LzFramesEntry), oSizes = oOff + 8 * T, oFrames = oSizes + 4 * T;
    size_t s;
    int rc;
    j->tableBytes = (oFrames + 4 * T + 7) & ~(size_t)7;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[0].h_aux, &c->stage[0].h_aux_cap, j->tableBytes))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[1].h_aux, &c->stage[1].h_aux_cap, F * sizeof(LzFramesResult)))) return rc;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, j->tableBytes + F * sizeof(LzFramesResult)))) return rc;
    for (s = 0; s < LZ_STAGES && s < j->nChunks; s++) {
        if ((rc = lzp_ensure_dev(c, (void**)&c->stage[s].d_slots, &c->stage[s].d_slots_cap, P * lz_bound_slot(j->maxBlock)))) return rc;
        if ((rc = lzp_ensure_dev(c, (void**)&c->stage[s].d_aux, &c->stage[s].d_aux_cap, b_aux_bytes(P)))) return rc;
    }
    j->h_frames = (LzFramesEntry*)c->stage[0].h_aux;         j->d_frames = (LzFramesEntry*)c->dfTab;
    j->h_blkOffsets = (uint64_t*)(c->stage[0].h_aux + oOff);  j->d_blkOffsets = (uint64_t*)(c->dfTab + oOff);
    j->h_blkSizes = (uint32_t*)(c->stage[0].h_aux + oSizes);  j->d_blkSizes = (uint32_t*)(c->dfTab + oSizes);
    j->h_blkFrames = (uint32_t*)(c->stage[0].h_aux + oFrames); j->d_blkFrames = (uint32_t*)(c->dfTab + oFrames);
    j->h_results = (LzFramesResult*)c->stage[1].h_aux;       j->d_results = (LzFramesResult*)(c->dfTab + j->tableBytes);
    j->A = c->stage[0].stream; j->B = c->stage[1].stream; j->C = c->stage[2].stream;
    return 0;
}

/* the per-frame and the per-block table, in pinned memory; a refused frame keeps its entry (so that indices stay the caller's) without
 * the LIVE flag, and no blocks */
static void b_tables(BJob* j)
{
    size_t i, b = 0;
    for (i = 0; i < j->nFrames; i++) {
        LzFramesEntry* e = &j->h_frames[i];
        LizardF_preferences_t prefs;
        size_t bs, nb, k;
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
        for (k = 0; k < nb; k++, b++) {
            j->h_blkOffsets[b] = (uint64_t)((const uint8_t*)j->srcs[i] + k * bs - j->base);
            j->h_blkSizes[b] = (uint32_t)(k + 1 == nb ? j->sizes[i] - k * bs : bs);
            j->h_blkFrames[b] = (uint32_t)i;
        }
    }
}

/* stream B starts behind what the caller's stream holds and uploads the tables; A and C start behind the upload */
static int b_upload(BJob* j, hipStream_t stream)
{
    LzStage* s = j->c->stage;
    LZ_HIP(hipEventRecord(s[0].up, stream));
    LZ_HIP(hipStreamWaitEvent(j->B, s[0].up, 0));
    LZ_HIP(hipMemcpyAsync(j->d_frames, j->h_frames, j->tableBytes, hipMemcpyHostToDevice, j->B));
    LZ_HIP(hipEventRecord(s[1].up, j->B));
    LZ_HIP(hipStreamWaitEvent(j->A, s[1].up, 0));
    LZ_HIP(hipStreamWaitEvent(j->C, s[1].up, 0));
    return 0;
}

/* every chunk, the hash, the finish and the copy of the result records: enqueued, nothing waited for */
static int b_enqueue(BJob* j)
{
    LzCtx* c = j->c;
    const size_t P = j->nBlocks < j->perChunk ? j->nBlocks : j->perChunk;
    size_t k;
    int rc;
    if (j->hash) {
        if ((rc = lzk_frames_hash_launch(j->d_frames, (uint32_t)j->nFrames, j->C))) return rc;
        LZ_HIP(hipEventRecord(c->stage[2].up, j->C));
    }
    for (k = 0; k < j->nChunks; k++) {
        LzStage* s = &c->stage[k % LZ_STAGES];
        const size_t first = k * j->perChunk, q = j->nBlocks - first < j->perChunk ? j->nBlocks - first : j->perChunk;
        uint32_t* const d_sizes = (uint32_t*)s->d_aux;
        uint64_t* const d_offsets = (uint64_t*)(s->d_aux + ((4 * P + 7) & ~(size_t)7));
        size_t bs = 0, b;
        for (b = first; b < first + q; b++) if (j->h_frames[j->h_blkFrames[b]].blockSize > bs) bs = j->h_frames[j->h_blkFrames[b]].blockSize;
        if (k >= LZ_STAGES) LZ_HIP(hipStreamWaitEvent(j->A, s->done, 0));      /* the slots and tables are free once chunk k - 3 is gathered */
        if ((rc = lzk_launch(c, j->base, q, bs, bs, s->d_slots, lz_bound_slot(bs), d_sizes, j->level, j->A, s->k0, s->k1, j->d_blkSizes + first,
                             j->d_blkOffsets + first))) return rc;
        LZ_HIP(hipStreamWaitEvent(j->B, s->k1, 0));
        if ((rc = lzk_frames_pack_launch(j->base, j->d_blkOffsets + first, j->d_blkSizes + first, j->d_blkFrames + first, s->d_slots, lz_bound_slot(bs),
                                         d_sizes, d_offsets, (uint32_t)q, j->d_frames, j->B))) return rc;
        LZ_HIP(hipEventRecord(s->done, j->B));
        c->devFrameCompressStats[2]++;
    }
    if (j->hash) LZ_HIP(hipStreamWaitEvent(j->B, c->stage[2].up, 0));
    if ((rc = lzk_frames_finish_launch(j->d_frames, j->d_results, (uint32_t)j->nFrames, j->B))) return rc;
    LZ_HIP(hipMemcpyAsync(j->h_results, j->d_results, j->nFrames * sizeof(LzFramesResult), hipMemcpyDeviceToHost, j->B));
    LZ_HIP(hipEventRecord(c->stage[0].meta, j->B));
    return 0;
}

/* the only wait of the call; then every live frame's answer */
static int b_collect(BJob* j)
{
    LzCtx* c = j->c;
    size_t i;
    LZ_HIP(hipEventSynchronize(c->stage[0].meta));
    for (i = 0; i < j->nFrames; i++) {
        const LzFramesResult* r = &j->h_results[i];
        if (j->results[i]) continue;
        if (r->size == LZK_FRAMES_OVERFLOW) { j->results[i] = LZ_FRAME_E(dstMaxSize_tooSmall); continue; }
        j->results[i] = (size_t)r->size;
        c->devFrameCompressStats[0] += (unsigned long long)j->h_frames[i].nBlocks - r->rawRecords;
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
    j.nFrames = nFrames; j.dsts = d_dsts; j.caps = dstCapacities; j.srcs = d_srcs; j.sizes = srcSizes; j.results = results; j.prefsPtr = preferencesPtr;
    /* every frame's refusal, before anything is enqueued; results[i] stays 0 for the frames that go on */
    for (i = 0; i < nFrames; i++) {
        results[i] = lzgpu_frame_device_plan(&prefs, preferencesPtr, d_dsts[i], dstCapacities[i], d_srcs[i], srcSizes[i]);
        if (results[i]) continue;
        {
            const size_t bs = lzgpu_frame_block_size((unsigned)prefs.frameInfo.blockSizeID), nb = (srcSizes[i] + bs - 1) / bs;
            live++;
            j.hash = prefs.frameInfo.contentChecksumFlag == 1;
            j.level = lzk_clamp_level(prefs.compressionLevel);
            if (!nb) continue;
            j.nBlocks += nb;
            if (bs > j.maxBlock) j.maxBlock = bs;
            if (!j.base || (const uint8_t*)d_srcs[i] < j.base) j.base = (const uint8_t*)d_srcs[i];
        }
    }
    if (!live) { b_first_refusal(nFrames, results); return 0; }
    if (j.nBlocks > 0xFFFFFFFFu) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (more than 2^32 - 1 blocks in one batch)");
        for (i = 0; i < nFrames; i++) if (!results[i]) results[i] = LZ_FRAME_E(GENERIC);
        return -LIZARDGPU_ERR_ARG;
    }
    lzk_guard_acquire(&g);
    rc = g.rc;
    if (!rc) {
        j.c = g.c;
        rc = lzk_ctx_init(g.c);
        if (!rc) {
            j.perChunk = lz_frame_chunk_blocks(g.c, j.maxBlock ? j.maxBlock : lzgpu_frame_block_size(1));
            j.nChunks = (j.nBlocks + j.perChunk - 1) / j.perChunk;
            rc = b_buffers(&j);
        }
        if (!rc) {
            b_tables(&j);
            g.c->hostKernelMs = -1.0f;
            rc = b_upload(&j, (hipStream_t)stream);
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
