/* lizard_stream_device.c — LizardGPU_compressStream_device: many buffers that lie in device memory, one Lizard frame each, written BACK TO
 * BACK into one device buffer, each behind an opaque prefix of the caller's (include/lizard_amd.h Part 3).  Plain C on the HIP
 * runtime's C API and the shim of lizard_gpu_ctx.h, in the shape of lizard_frames_device.c, whose third form it is: one frame and one
 * position (lizard_frame_device.c), many frames and many destinations (lizard_frames_device.c), many frames and ONE destination.
 * Frame i is byte for byte what LizardGPU_compressFrame_device writes for that buffer with LizardGPU_compressFrameBound + 8 bytes of
 * room: the refusals are lzgpu_frame_device_plan's (lizard_frame_host.c), the header is lzgpu_frame_write_header's, the records are
 * the same block kernels' — but a refusal stops the call before anything is launched, because a stream with a hole is not a stream.
 *
 * The position rule.  Frame i starts where frame i - 1 ends, and only the device knows where that is.  What does not depend on
 * compressed sizes the host adds up per frame (LzStreamEntry::fixed: the prefixes and headers up to and including the frame's own, the
 * end marks and checksum words of the frames before it); the record bytes of all blocks in front of a record are a plain prefix sum
 * carried from chunk to chunk in ONE word of device memory (lz_stream_scan_kernel, lz_stream_pack.h).  The blocks of all frames form
 * one list in frame order, cut into chunks as in lizard_frames_device.c (lz_frame_chunk_blocks, LIZARDGPU_FRAME_CHUNK_BLOCKS); each
 * chunk is one ragged launch of the block kernels into a stage's slots (stream A), scanned and gathered on stream B — the gather is
 * lz_frames_gather_kernel unchanged, over a table whose entries all name d_dst with the capacity as their limit.  The three stages
 * rotate under events.  With a checksum lz_xxh32_frames_kernel hashes every source on the device (stream C).  lz_stream_finish_kernel
 * (stream B, behind the last gather and the hash) writes prefixes, headers, end marks and checksum words, the frame offsets and the
 * result record.  All of it is enqueued before the host waits for anything; the host waits once.
 *
 * What crosses PCIe: going up, one copy of 16 + 144 bytes per frame + 16 per block + the prefix bytes; coming down, 16 bytes and,
 * when the caller asks for them, 8 per frame + 8.  No payload byte in either direction, checksum or not. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_batch.h"

#define LZ_STREAM_SLACK 8      /* what every frame gets beyond LizardGPU_compressFrameBound (its known shortfall is 5 bytes) */

typedef struct {
    LzBatch b;                                                /* the blocks of all frames as one list (lizard_device_batch.h) */
    size_t prefixTotal, capacity;
    void* dst; const void* const* srcs; const size_t* sizes; const void* const* prefixes; const size_t* prefixSizes;
    const LizardF_preferences_t* prefsPtr;
    uint64_t* frameOffsets;
    uint64_t fixedTotal;                                      /* every prefix, header, end mark and checksum word of the call, and extraFixed */
    uint64_t extraFixed;                                      /* bytes the caller of lzgpu_stream_compress writes behind the last frame */
    lzgpu_stream_after_fn after; void* afterArg;              /* ... from this hook: enqueued on stream B behind the finish kernel */
    int launched;
    /* what goes up, in pinned memory (stage 0's h_aux) and in the same layout in device memory (LzCtx::dfTab): the state, the two
     * frame tables, the block tables, the prefix bytes; behind them in dfTab the result record and the frame offsets, which come
     * down into stage 1's h_aux */
    size_t upBytes, downBytes;
    LzStreamState *h_state, *d_state;
    LzStreamEntry *h_entries, *d_entries;
    uint8_t *h_blob, *d_blob;
    LzFramesResult *h_result, *d_result;
    uint64_t *h_offsets, *d_offsets;
} SJob;

static int s_buffers(SJob* j)
{
    LzBatch* b = &j->b;
    LzCtx* c = b->c;
    const size_t F = b->nFrames;
    const size_t oFrames = sizeof(LzStreamState), oEntries = oFrames + F * sizeof(LzFramesEntry), oOff = oEntries + F * sizeof(LzStreamEntry),
                 oBlob = lz_batch_tables_end(b, oOff);
    int rc;
    j->upBytes = (oBlob + j->prefixTotal + 8) & ~(size_t)7;                       /* (never empty behind oBlob: the blob's address is a valid one) */
    j->downBytes = sizeof(LzFramesResult) + (j->frameOffsets ? 8 * (F + 1) : 0);
    if ((rc = lzp_ensure_pinned((void**)&c->stage[0].h_aux, &c->stage[0].h_aux_cap, j->upBytes))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[1].h_aux, &c->stage[1].h_aux_cap, sizeof(LzFramesResult) + 8 * (F + 1)))) return rc;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, j->upBytes + sizeof(LzFramesResult) + 8 * (F + 1)))) return rc;
    if ((rc = lz_batch_stages(b))) return rc;
    j->h_state = (LzStreamState*)c->stage[0].h_aux;                  j->d_state = (LzStreamState*)c->dfTab;
    b->h_frames = (LzFramesEntry*)(c->stage[0].h_aux + oFrames);     b->d_frames = (LzFramesEntry*)(c->dfTab + oFrames);
    j->h_entries = (LzStreamEntry*)(c->stage[0].h_aux + oEntries);   j->d_entries = (LzStreamEntry*)(c->dfTab + oEntries);
    lz_batch_block_tables(b, c->stage[0].h_aux, c->dfTab, oOff);
    j->h_blob = c->stage[0].h_aux + oBlob;                           j->d_blob = c->dfTab + oBlob;
    j->h_result = (LzFramesResult*)c->stage[1].h_aux;                j->d_result = (LzFramesResult*)(c->dfTab + j->upBytes);
    j->h_offsets = (uint64_t*)(c->stage[1].h_aux + sizeof(LzFramesResult));
    j->d_offsets = (uint64_t*)(c->dfTab + j->upBytes + sizeof(LzFramesResult));
    return 0;
}

/* the state, the per-frame and the per-block tables and the prefix bytes, in pinned memory */
static void s_tables(SJob* j)
{
    const size_t F = j->b.nFrames;
    size_t i, b = 0, blob = 0;
    uint64_t fixed = 0;
    uint32_t next = (uint32_t)F;
    memset(j->h_state, 0, sizeof *j->h_state);
    for (i = 0; i < F; i++) {
        LzFramesEntry* e = &j->b.h_frames[i];
        LzStreamEntry* s = &j->h_entries[i];
        LizardF_preferences_t prefs;
        const size_t pre = j->prefixSizes ? j->prefixSizes[i] : 0;
        size_t bs, nb;
        memset(e, 0, sizeof *e);
        memset(s, 0, sizeof *s);
        (void)lzgpu_frame_device_plan(&prefs, j->prefsPtr, j->dst, LizardGPU_compressFrameBound(j->sizes[i], j->prefsPtr) + LZ_STREAM_SLACK, j->srcs[i],
                                      j->sizes[i]);
        bs = lzgpu_frame_block_size((unsigned)prefs.frameInfo.blockSizeID);
        nb = (j->sizes[i] + bs - 1) / bs;
        e->dst = (uint64_t)(uintptr_t)j->dst;
        e->limit = (uint64_t)j->capacity;
        e->headerBytes = (uint32_t)lzgpu_frame_write_header(e->header, &prefs.frameInfo);
        e->src = (uint64_t)(uintptr_t)j->srcs[i]; e->srcSize = (uint64_t)j->sizes[i];
        e->blockSize = (uint32_t)bs; e->nBlocks = (uint32_t)nb;
        e->flags = LZK_FRAMES_LIVE | (prefs.frameInfo.contentChecksumFlag == 1 ? LZK_FRAMES_CHECKSUM : 0u);
        s->prefixOff = (uint64_t)blob; s->prefixBytes = (uint64_t)pre;
        if (pre) memcpy(j->h_blob + blob, j->prefixes[i], pre);
        blob += pre;
        fixed += pre + e->headerBytes;
        s->fixed = fixed;
        s->tailBytes = 4u + (prefs.frameInfo.contentChecksumFlag == 1 ? 4u : 0u);
        fixed += s->tailBytes;
        s->firstBlock = nb ? (uint32_t)b : 0xFFFFFFFFu;
        s->lastBlock = nb ? (uint32_t)(b + nb - 1) : 0xFFFFFFFFu;
        lz_batch_blocks(&j->b, &b, i, j->srcs[i], j->sizes[i], bs, nb);
    }
    j->fixedTotal = fixed + j->extraFixed;
    for (i = F; i-- > 0;) {                                  /* the first frame with blocks at or behind / behind each frame */
        j->h_entries[i].nextAfter = next;
        if (j->b.h_frames[i].nBlocks) next = (uint32_t)i;
        j->h_entries[i].nextSelf = next;
    }
}

/* a chunk's records get their places behind the carry and move there (lz_batch_rotate's pack) */
static int s_pack(void* arg, const LzBatch* b, const LzStage* s, size_t first, size_t q, size_t bs, uint32_t* d_sizes, uint64_t* d_offsets)
{
    const SJob* j = (const SJob*)arg;
    return lzk_stream_pack_launch(b->base, b->d_blkOffsets + first, b->d_blkSizes + first, b->d_blkFrames + first, s->d_slots, lz_bound_slot(bs), d_sizes,
                                  d_offsets, (uint32_t)q, (uint32_t)first, b->d_frames, j->d_entries, j->d_state, (uint64_t)j->capacity, b->B);
}

/* every chunk, the hash, the finish and the copy of the result record and the offsets: enqueued, nothing waited for */
static int s_enqueue(SJob* j)
{
    LzBatch* b = &j->b;
    LzCtx* c = b->c;
    int rc;
    if ((rc = lz_batch_rotate(b, s_pack, j, &c->devStreamCompressStats[2], &j->launched))) return rc;
    if ((rc = lzk_stream_finish_launch(b->d_frames, j->d_entries, j->d_blob, j->d_state, (uint32_t)b->nFrames, j->fixedTotal, (uint64_t)j->capacity,
                                       j->d_result, j->d_offsets, b->B))) return rc;
    j->launched = 1;
    if (j->after && (rc = j->after(j->afterArg, b->d_frames, j->d_entries, j->d_state, j->d_offsets, (uint32_t)b->nFrames, j->fixedTotal,
                                   (uint64_t)j->capacity, b->B))) return rc;
    LZ_HIP(hipMemcpyAsync(j->h_result, j->d_result, j->downBytes, hipMemcpyDeviceToHost, b->B));
    LZ_HIP(hipEventRecord(c->stage[0].meta, b->B));
    return 0;
}

size_t LizardGPU_compressStreamBound(size_t nFrames, const size_t* srcSizes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs)
{
    size_t i, sum = 0;
    if (nFrames && !srcSizes) return LZ_FRAME_E(GENERIC);
    for (i = 0; i < nFrames; i++) {
        const size_t b = LizardGPU_compressFrameBound(srcSizes[i], prefs), add = b + LZ_STREAM_SLACK + (prefixSizes ? prefixSizes[i] : 0);
        if (LizardGPU_frameIsError(b) || add < b || sum + add < sum) return LZ_FRAME_E(GENERIC);
        sum += add;
    }
    return LizardGPU_frameIsError(sum) ? LZ_FRAME_E(GENERIC) : sum;
}

/* LizardGPU_compressStream_device with room for something behind the last frame: extraFixed bytes join the bytes the host knows
 * (the returned size, frameOffsets[nFrames] and the one capacity test count them), and `after` (may be NULL) is called once, behind
 * the launch of lz_stream_finish_kernel, to enqueue on stream B what writes them; it sees the device tables of the call.  With
 * (0, NULL, NULL) this is the public entry, launch for launch.  lizard_seek_device.c puts the seek table there. */
size_t lzgpu_stream_compress(void* d_dst, size_t dstCapacity, size_t nFrames, const void* const* d_srcs, const size_t* srcSizes,
                             const void* const* prefixes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs,
                             uint64_t* frameOffsets, size_t* failedFrame, void* stream, uint64_t extraFixed, lzgpu_stream_after_fn after,
                             void* afterArg)
{
    LizardF_preferences_t plan;
    SJob j;
    LzGuard g;
    size_t i, result = 0;
    uint64_t fixed = extraFixed;
    int rc;
    lzk_err()[0] = 0;
    if (!nFrames) return 0;
    if (!d_dst || !d_srcs || !srcSizes || !prefixes != !prefixSizes || nFrames > 0x7FFFFFFFu) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null array, prefixes without their sizes, or more than 2^31 - 1 frames)");
        return LZ_FRAME_E(GENERIC);
    }
    memset(&j, 0, sizeof j);
    j.b.nFrames = nFrames; j.dst = d_dst; j.capacity = dstCapacity; j.srcs = d_srcs; j.sizes = srcSizes; j.prefixes = prefixes; j.prefixSizes = prefixSizes;
    j.prefsPtr = prefs; j.frameOffsets = frameOffsets;
    j.extraFixed = extraFixed; j.after = after; j.afterArg = afterArg;
    /* the first frame in index order that the single-frame entry would refuse decides, before anything is enqueued */
    for (i = 0; i < nFrames; i++) {
        const size_t pre = prefixSizes ? prefixSizes[i] : 0;
        size_t code = lzgpu_frame_device_plan(&plan, prefs, d_dst, LizardGPU_compressFrameBound(srcSizes[i], prefs) + LZ_STREAM_SLACK, d_srcs[i], srcSizes[i]);
        if (!code && pre && !prefixes[i]) code = LZ_FRAME_E(GENERIC);
        if (code) {
            if (failedFrame) *failedFrame = i;
            snprintf(lzk_err(), LZK_ERR_BYTES, "frame %zu refused: %s", i, code == LZ_FRAME_E(GENERIC) ? "bad argument (null pointer)" : LizardF_getErrorName(code));
            return code;
        }
        {
            const size_t bs = lzgpu_frame_block_size((unsigned)plan.frameInfo.blockSizeID), nb = (srcSizes[i] + bs - 1) / bs;
            uint8_t header[20];
            j.b.hash = plan.frameInfo.contentChecksumFlag == 1;
            j.b.level = lzk_clamp_level(plan.compressionLevel);
            j.prefixTotal += pre;
            fixed += pre + lzgpu_frame_write_header(header, &plan.frameInfo) + 4u + (j.b.hash ? 4u : 0u);
            if (!nb) continue;
            j.b.nBlocks += nb;
            if (bs > j.b.maxBlock) j.b.maxBlock = bs;
            if (!j.b.base || (const uint8_t*)d_srcs[i] < j.b.base) j.b.base = (const uint8_t*)d_srcs[i];
        }
    }
    if (j.b.nBlocks > 0xFFFFFFFFu) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (more than 2^32 - 1 blocks in one stream)");
        return LZ_FRAME_E(GENERIC);
    }
    if (fixed > dstCapacity) {                               /* prefixes, headers and tails alone do not fit: nothing to launch */
        snprintf(lzk_err(), LZK_ERR_BYTES, "the stream needs more than dstCapacity = %zu bytes", dstCapacity);
        return LZ_FRAME_E(dstMaxSize_tooSmall);
    }
    if (!j.b.base) j.b.base = (const uint8_t*)d_dst;             /* (no frame has a block: no launch reads through it) */
    lzk_guard_acquire(&g);
    rc = g.rc;
    if (!rc) {
        j.b.c = g.c;
        rc = lzk_ctx_init(g.c);
        if (!rc) {
            j.b.perChunk = lz_frame_chunk_blocks(g.c, j.b.maxBlock ? j.b.maxBlock : lzgpu_frame_block_size(1));
            j.b.nChunks = (j.b.nBlocks + j.b.perChunk - 1) / j.b.perChunk;
            rc = s_buffers(&j);
        }
        if (!rc) {
            s_tables(&j);
            g.c->hostKernelMs = -1.0f;
            rc = lz_batch_upload(&j.b, j.d_state, j.h_state, j.upBytes, (hipStream_t)stream);
        }
        if (!rc) rc = s_enqueue(&j);
        if (!rc) {                                           /* the only wait of the call */
            const hipError_t e = hipEventSynchronize(g.c->stage[0].meta);
            if (e != hipSuccess) { snprintf(lzk_err(), LZK_ERR_BYTES, "hipEventSynchronize failed: %s", hipGetErrorString(e)); rc = -LIZARDGPU_ERR_HIP; }
        }
        if (j.launched) g.c->devStreamCompressStats[3]++;
        if (!rc) {
            if (j.h_result->size == LZK_FRAMES_OVERFLOW) {
                snprintf(lzk_err(), LZK_ERR_BYTES, "the stream needs more than dstCapacity = %zu bytes", dstCapacity);
                result = LZ_FRAME_E(dstMaxSize_tooSmall);
            } else {
                result = (size_t)j.h_result->size;
                g.c->devStreamCompressStats[0] += nFrames;
                g.c->devStreamCompressStats[1] += j.h_result->rawRecords;
                if (frameOffsets) memcpy(frameOffsets, j.h_offsets, 8 * (nFrames + 1));
            }
        }
        lz_quiesce(g.c);
        lzk_guard_release(&g);
    }
    return rc ? LZ_FRAME_E(GENERIC) : result;
}

size_t LizardGPU_compressStream_device(void* d_dst, size_t dstCapacity, size_t nFrames, const void* const* d_srcs, const size_t* srcSizes,
                                       const void* const* prefixes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs,
                                       uint64_t* frameOffsets, size_t* failedFrame, void* stream)
{
    return lzgpu_stream_compress(d_dst, dstCapacity, nFrames, d_srcs, srcSizes, prefixes, prefixSizes, prefs, frameOffsets, failedFrame, stream, 0, NULL,
                                 NULL);
}

int LizardGPU_streamCompressDeviceStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devStreamCompressStats));
}
