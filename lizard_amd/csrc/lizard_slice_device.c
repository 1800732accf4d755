/* lizard_slice_device.c — a row range of a tensor out of a stream in device memory (include/lizard_amd.h Part 3d):
 * LizardGPU_decompressFrameRanges_device decodes, of a batch of frames, only the records that cover the byte ranges a caller asks for,
 * and LizardGPU_joinPlanesRange_device joins an element range out of pieces of its planes.  Plain C on the HIP runtime's C API and the
 * shim of lizard_gpu_ctx.h, like the sibling device entries; the arithmetic both rest on is lizard_slice_host.c.
 *
 * LizardGPU_decompressFrameRanges_device waits twice per CALL, like the batch decoder whose walk it reuses:
 *   count pass   one table entry per frame goes up; lz_unframes_walk_kernel (unframes_kernels.h, unchanged) walks every frame, one
 *                wave each; one LzWalkResult per frame comes down.  The host answers what is decided now — a chain the walk refuses,
 *                a skippable frame, a frame whose header or ranges do not fit the rule "record x / B holds byte x" — gives every
 *                range of the other frames its place in d_dst (whole blocks, back to back, in index order), tests the total
 *                against dstCapacity, and turns the ranges into ONE list of picked records.
 *   fill pass    the same walk again, writing the payload offsets and record words of every frame that has a pick; ONE launch of
 *                lz_unslice_kernel (unslice_kernels.h) over the picks; the per-pick results come down.  A pick that did not decode to
 *                exactly what its place in the frame demands fails its frame: decompressionFailed.
 * Nothing is delegated: a frame this entry cannot answer from its picked records alone is refused, never decoded whole.
 *
 * LizardGPU_joinPlanesRange_device is the call of lizard_planes_device.c: the arguments are checked before anything is touched, the
 * non-empty items become the entries of a table with the piece addresses behind it, the table goes up from pinned memory and the
 * kernel (planes_range_kernels.h) runs, both on the caller's stream; the host waits once. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_batch.h"
#include "unslice_kernels.h"
#include "planes_range_kernels.h"

enum { S_OPEN = 0, S_DECIDED = 1 };
#define S_NO_OWNER 0xFFFFFFFFu

typedef struct {
    LzCtx* c;
    size_t nFrames, nRanges, nRecords, nPicks;
    const LizardGPU_sliceFrame_t* frames; const LizardGPU_byteRange_t* ranges;
    unsigned char* state;                                     /* S_*, one per frame */
    uint32_t* owner;                                          /* the frame of every range, or S_NO_OWNER */
    LzWalkResult* walk;                                       /* the count pass's results, out of the pinned buffer (which the fill pass's tables may move) */
    /* what goes up, in pinned memory (stage 0's h_aux) and in the same layout at the head of LzCtx::dfTab: the frame table and the
     * picks; behind them in dfTab only: walk results and per-pick results (both come down into stage 1's h_aux), payload offsets,
     * record words */
    size_t upBytes;
    LzUnframesEntry *h_frames, *d_frames;
    LzSlicePick *h_picks, *d_picks;
    LzWalkResult *h_walk, *d_walk;
    uint32_t *h_out, *d_out;
    uint64_t* d_offs; uint32_t* d_words;
    hipStream_t S;
} SJob;

static int s_buffers(SJob* j, size_t R, size_t K)
{
    LzCtx* c = j->c;
    const size_t F = j->nFrames;
    const size_t oPicks = F * sizeof(LzUnframesEntry), oWalk = oPicks + K * sizeof(LzSlicePick), oOffs = oWalk + F * sizeof(LzWalkResult);
    const size_t oWords = oOffs + 8 * R, oOut = oWords + 4 * R;
    int rc;
    j->upBytes = oWalk;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[0].h_aux, &c->stage[0].h_aux_cap, j->upBytes))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[1].h_aux, &c->stage[1].h_aux_cap, F * sizeof(LzWalkResult) + 4 * K))) return rc;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, oOut + 4 * K))) return rc;
    j->h_frames = (LzUnframesEntry*)c->stage[0].h_aux;        j->d_frames = (LzUnframesEntry*)c->dfTab;
    j->h_picks = (LzSlicePick*)(c->stage[0].h_aux + oPicks);  j->d_picks = (LzSlicePick*)(c->dfTab + oPicks);
    j->h_walk = (LzWalkResult*)c->stage[1].h_aux;             j->d_walk = (LzWalkResult*)(c->dfTab + oWalk);
    j->h_out = (uint32_t*)(c->stage[1].h_aux + F * sizeof(LzWalkResult)); j->d_out = (uint32_t*)(c->dfTab + oOut);
    j->d_offs = (uint64_t*)(c->dfTab + oOffs); j->d_words = (uint32_t*)(c->dfTab + oWords);
    j->S = c->stage[1].stream;
    return 0;
}

/* what the header and the ranges of an open frame say against the rule that byte x lies in record x / B: 0, or the frame's code */
static size_t s_judge(const SJob* j, size_t f, const LzWalkResult* w)
{
    const uint64_t B = (uint64_t)lzgpu_frame_block_size(w->blockSizeID), C = w->contentSize;
    uint32_t r;
    if (w->status) return (size_t)-(long)w->status;
    if (w->frameType) return LZ_FRAME_E(frameType_unknown);
    if (!B || (w->nRecords && !C) || w->nRecords != (C + B - 1) / B) return LZ_FRAME_E(frameSize_wrong);
    for (r = 0; r < j->frames[f].nRanges; r++) {
        const LizardGPU_byteRange_t* x = &j->ranges[j->frames[f].firstRange + r];
        if (x->lo > x->hi || x->hi > C) return LZ_FRAME_E(frameSize_wrong);
    }
    return 0;
}

/* The call under the context guard.  0, or -LIZARDGPU_ERR_*; on 0 every frame is answered. */
static int s_batch(SJob* j, void* d_dst, size_t dstCapacity, uint64_t* rangeAt, size_t* results, hipStream_t stream)
{
    LzCtx* c = j->c;
    uint64_t place = 0, picks = 0, records = 0;
    size_t i, r, k;
    int rc;
    if ((rc = lzk_ctx_init(c))) return rc;
    if ((rc = s_buffers(j, 0, 0))) return rc;
    c->hostKernelMs = -1.0f;
    if ((rc = lz_count_pass(c, j->nFrames, j->state, &j->frames[0].d_src, sizeof j->frames[0], &j->frames[0].srcSize, sizeof j->frames[0], j->h_frames,
                            j->d_frames, j->h_walk, j->d_walk, j->S, stream))) return rc;
    c->devSliceStats[3]++;
    memcpy(j->walk, j->h_walk, j->nFrames * sizeof *j->walk);
    for (i = 0; i < j->nFrames; i++) {
        if (j->state[i] != S_OPEN) continue;
        if ((results[i] = s_judge(j, i, &j->walk[i]))) j->state[i] = S_DECIDED;
    }
    /* every range's place: whole blocks, back to back, in index order; the ranges of a refused frame, and of no frame, take no room */
    for (r = 0; r < j->nRanges; r++) {
        const uint32_t f = j->owner[r];
        rangeAt[r] = place;
        if (f == S_NO_OWNER || j->state[f] != S_OPEN || j->ranges[r].hi <= j->ranges[r].lo) continue;
        {
            const uint64_t B = (uint64_t)lzgpu_frame_block_size(j->walk[f].blockSizeID);
            const uint64_t blocks = (j->ranges[r].hi - 1) / B + 1 - j->ranges[r].lo / B;
            if (blocks > (~(uint64_t)0 - place) / B) { place = ~(uint64_t)0; break; }
            place += blocks * B; picks += blocks;
        }
    }
    if (r < j->nRanges || place > (uint64_t)dstCapacity || (place && !d_dst)) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "dstMaxSize_tooSmall: the covering blocks of the ranges take %llu bytes, dstCapacity = %zu%s",
                 (unsigned long long)place, dstCapacity, place && !d_dst ? " (d_dst is null)" : "");
        return -LIZARDGPU_ERR_ARG;
    }
    rangeAt[j->nRanges] = place;
    for (i = 0; i < j->nFrames; i++) {                         /* the record tables hold the frames that have a pick */
        const LizardGPU_sliceFrame_t* x = &j->frames[i];
        int any = 0;
        if (j->state[i] != S_OPEN) continue;
        for (r = 0; r < x->nRanges; r++) any |= j->ranges[x->firstRange + r].hi > j->ranges[x->firstRange + r].lo;
        if (any) records += j->walk[i].nRecords;
        else { results[i] = 0; j->state[i] = S_DECIDED; c->devSliceStats[1]++; }
    }
    if (picks > 0xFFFFFFFFull || records > 0xFFFFFFFFull) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (2^32 or more block records in one call)");
        return -LIZARDGPU_ERR_ARG;
    }
    j->nPicks = (size_t)picks; j->nRecords = (size_t)records;
    if (j->nPicks) {
        size_t first = 0;
        if ((rc = s_buffers(j, j->nRecords, j->nPicks))) return rc;
        for (i = 0, k = 0; i < j->nFrames; i++) {              /* (the pinned table may have moved since the count pass) */
            const LizardGPU_sliceFrame_t* x = &j->frames[i];
            const LzWalkResult* w = &j->walk[i];
            LzUnframesEntry* e = &j->h_frames[i];
            const uint64_t B = (uint64_t)lzgpu_frame_block_size(w->blockSizeID);
            memset(e, 0, sizeof *e);
            if (j->state[i] != S_OPEN) continue;
            lz_fill_entry(e, x->d_src, x->srcSize, first, w);
            for (r = 0; r < x->nRanges; r++) {
                const LizardGPU_byteRange_t* g = &j->ranges[x->firstRange + r];
                uint64_t b;
                if (g->hi <= g->lo) continue;
                for (b = g->lo / B; b <= (g->hi - 1) / B; b++, k++) {
                    LzSlicePick* p = &j->h_picks[k];
                    p->dstOff = rangeAt[x->firstRange + r] + (b - g->lo / B) * B;
                    p->rec = (uint32_t)(first + b); p->frame = (uint32_t)i;
                    p->want = (uint32_t)(b + 1 < w->nRecords ? B : w->contentSize - b * B);
                    p->reserved = 0;
                }
            }
            first += (size_t)w->nRecords;
        }
        LZ_HIP(hipMemcpyAsync(j->d_frames, j->h_frames, j->upBytes, hipMemcpyHostToDevice, j->S));
        if ((rc = lzk_unframes_walk_launch(j->d_frames, (uint32_t)j->nFrames, 1, j->d_offs, j->d_words, j->d_walk, j->S))) return rc;
        if ((rc = lzk_unslice_launch(c, j->d_frames, j->d_offs, j->d_words, j->d_picks, d_dst, j->d_out, j->nPicks, j->S))) return rc;
        LZ_HIP(hipMemcpyAsync(j->h_out, j->d_out, 4 * j->nPicks, hipMemcpyDeviceToHost, j->S));
        LZ_HIP(hipEventRecord(c->stage[0].meta, j->S));
        LZ_HIP(hipEventSynchronize(c->stage[0].meta));
        for (k = 0; k < j->nPicks; k++)
            if (j->h_out[k] != j->h_picks[k].want) results[j->h_picks[k].frame] = LZ_FRAME_E(decompressionFailed);
        c->devSliceStats[0] += j->nPicks;
    }
    for (i = 0; i < j->nFrames; i++) {
        if (j->state[i] == S_OPEN) { c->devSliceStats[results[i] ? 2 : 1]++; j->state[i] = S_DECIDED; }
        else if (results[i]) c->devSliceStats[2]++;
    }
    return 0;
}

int LizardGPU_decompressFrameRanges_device(void* d_dst, size_t dstCapacity, size_t nFrames, const LizardGPU_sliceFrame_t* frames,
                                           const LizardGPU_byteRange_t* ranges, uint64_t* rangeAt, size_t* results, void* stream)
{
    SJob j;
    LzGuard g;
    size_t i, r, open = 0;
    int rc = 0;
    lzk_err()[0] = 0;
    if (!rangeAt) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null rangeAt)"); return -LIZARDGPU_ERR_ARG; }
    rangeAt[0] = 0;
    if (!nFrames) return 0;
    if (!frames || !results || nFrames >= S_NO_OWNER) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null array or 2^32 or more frames)");
        return -LIZARDGPU_ERR_ARG;
    }
    memset(&j, 0, sizeof j);
    j.nFrames = nFrames; j.frames = frames; j.ranges = ranges;
    for (i = 0; i < nFrames; i++) {
        const size_t end = (size_t)frames[i].firstRange + frames[i].nRanges;
        results[i] = LZ_FRAME_E(GENERIC);
        if (frames[i].nRanges && end > j.nRanges) j.nRanges = end;
    }
    if (j.nRanges && !ranges) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null ranges)"); return -LIZARDGPU_ERR_ARG; }
    for (r = 0; r <= j.nRanges; r++) rangeAt[r] = 0;
    j.state = (unsigned char*)calloc(nFrames, 1);
    j.owner = (uint32_t*)malloc((j.nRanges + 1) * sizeof *j.owner);
    j.walk = (LzWalkResult*)malloc(nFrames * sizeof *j.walk);
    if (!j.state || !j.owner || !j.walk) {
        free(j.state); free(j.owner); free(j.walk);
        snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory");
        return -LIZARDGPU_ERR_NOMEM;
    }
    for (r = 0; r < j.nRanges; r++) j.owner[r] = S_NO_OWNER;
    for (i = 0; i < nFrames && !rc; i++) {
        for (r = 0; r < frames[i].nRanges; r++) {
            if (j.owner[frames[i].firstRange + r] != S_NO_OWNER) {
                snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (range %zu belongs to frame %u and to frame %zu)", (size_t)frames[i].firstRange + r,
                         (unsigned)j.owner[frames[i].firstRange + r], i);
                rc = -LIZARDGPU_ERR_ARG;
                break;
            }
            j.owner[frames[i].firstRange + r] = (uint32_t)i;
        }
        if (!frames[i].d_src && frames[i].srcSize) j.state[i] = S_DECIDED;        /* GENERIC */
        else open++;
    }
    if (!rc && open) {
        lzk_guard_acquire(&g);
        rc = g.rc;
        if (!rc) {
            j.c = g.c;
            rc = s_batch(&j, d_dst, dstCapacity, rangeAt, results, (hipStream_t)stream);
            lz_quiesce(g.c);
            lzk_guard_release(&g);
        }
    }
    if (rc) {
        for (i = 0; i < nFrames; i++) if (!LizardGPU_frameIsError(results[i])) results[i] = LZ_FRAME_E(GENERIC);
    } else lz_first_refusal(nFrames, results);
    free(j.state);
    free(j.owner);
    free(j.walk);
    return rc;
}

int LizardGPU_sliceDeviceStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devSliceStats));
}

/* ---- the range join ---- */

#define R_MAX_PIECES 65                                        /* 8 * 8 planes and the raw elements */

static int r_locked(LzCtx* c, const void* tab, size_t nEntries, size_t nPieces, uint32_t nTiles, hipStream_t stream)
{
    const size_t oPieces = nEntries * sizeof(LzPlanesRangeEntry);
    int rc;
    if ((rc = lz_table_upload(c, tab, oPieces + 8 * nPieces, stream))) return rc;
    if ((rc = lzk_planes_range_launch(c, (const LzPlanesRangeEntry*)c->dfTab, (uint32_t)nEntries, (const uint64_t*)(c->dfTab + oPieces), nTiles, stream))) return rc;
    LZ_HIP(hipStreamSynchronize(stream));
    return 0;
}

int LizardGPU_joinPlanesRange_device(size_t nItems, const LizardGPU_planesRange_t* items, const void* const* d_pieces, void* stream)
{
    LizardGPU_byteRange_t ranges[R_MAX_PIECES];
    LzPlanesRangeEntry* tab;
    uint64_t* pieces;
    uint8_t* mem;
    LzGuard g;
    uint64_t tiles = 0;
    size_t i, q, live = 0, nPieces = 0;
    int rc;
    if (!nItems) return 0;
    lzk_err()[0] = 0;
    if (!items || !d_pieces) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null array)"); return -LIZARDGPU_ERR_ARG; }
    for (i = 0; i < nItems; i++) {
        const LizardGPU_planesRange_t* x = &items[i];
        const size_t n = LizardGPU_planesRangeBytes(x->nElems, x->elemSize, x->filter, x->first, x->last, ranges, R_MAX_PIECES);
        if (!n || x->reserved) {
            snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (item %zu: element size %u, filter %u, elements [%llu, %llu) of %llu)", i, (unsigned)x->elemSize,
                     (unsigned)x->filter, (unsigned long long)x->first, (unsigned long long)x->last, (unsigned long long)x->nElems);
            return -LIZARDGPU_ERR_ARG;
        }
        if (x->first == x->last) continue;
        for (q = 0; q < n; q++)
            if (ranges[q].hi > ranges[q].lo && !d_pieces[x->firstPiece + q]) break;
        if (!x->d_dst || q < n) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (item %zu: null pointer)", i); return -LIZARDGPU_ERR_ARG; }
        tiles += ((x->last - (x->filter ? x->first & ~(uint64_t)7 : x->first)) * x->elemSize + LZP_TILE_BYTES - 1) / LZP_TILE_BYTES;
        nPieces += n;
        live++;
    }
    if (tiles >> 32) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (the batch has 2^32 tiles of %u bytes or more)", LZP_TILE_BYTES); return -LIZARDGPU_ERR_ARG; }
    if (!live) return 0;                                        /* nothing but empty items: nothing to move */
    mem = (uint8_t*)malloc(live * sizeof *tab + 8 * nPieces);
    if (!mem) { snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); return -LIZARDGPU_ERR_NOMEM; }
    tab = (LzPlanesRangeEntry*)mem; pieces = (uint64_t*)(mem + live * sizeof *tab);
    for (i = 0, live = 0, tiles = 0, nPieces = 0; i < nItems; i++) {
        const LizardGPU_planesRange_t* x = &items[i];
        const size_t n = x->filter ? 8 * (size_t)x->elemSize + 1 : x->elemSize;
        LzPlanesRangeEntry* e = &tab[live];
        if (x->first == x->last) continue;
        e->dst = (uint64_t)(uintptr_t)x->d_dst; e->base = (uint64_t)(uintptr_t)x->d_base;
        e->nElems = x->nElems; e->first = x->first; e->last = x->last;
        e->elem = x->elemSize; e->filter = x->filter; e->firstTile = (uint32_t)tiles; e->firstPiece = (uint32_t)nPieces;
        for (q = 0; q < n; q++) pieces[nPieces + q] = (uint64_t)(uintptr_t)d_pieces[x->firstPiece + q];
        tiles += ((x->last - (x->filter ? x->first & ~(uint64_t)7 : x->first)) * x->elemSize + LZP_TILE_BYTES - 1) / LZP_TILE_BYTES;
        nPieces += n;
        live++;
    }
    lzk_guard_acquire(&g);
    if (g.rc) { free(mem); return g.rc; }
    rc = r_locked(g.c, mem, live, nPieces, (uint32_t)tiles, (hipStream_t)stream);
    if (rc) lz_drain_caller((hipStream_t)stream);
    lzk_guard_release(&g);
    free(mem);
    return rc;
}
