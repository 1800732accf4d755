/* lizard_device_batch.h — what the batch entries on device memory share, beside lizard_device_common.h: the error text of a batch
 * that did its work, the count pass of the frame-batch walk (lizard_unframes_device.c, lizard_slice_device.c) and the chunk list of
 * the batch compressors (lizard_frames_device.c, lizard_stream_device.c): its stage buffers, its block tables, its upload and the
 * rotation of its stages under events.  Private, plain C, static inline: a file takes what it uses. */
#ifndef LIZARD_DEVICE_BATCH_H
#define LIZARD_DEVICE_BATCH_H
#include "lizard_device_common.h"
#include "unframes_kernels.h"

/* the error text of a call that did its work: the first frame that was refused, or none */
static inline void lz_first_refusal(size_t nFrames, const size_t* results)
{
    size_t i;
    for (i = 0; i < nFrames; i++)
        if (LizardGPU_frameIsError(results[i])) {
            snprintf(lzk_err(), LZK_ERR_BYTES, "frame %zu refused: %s", i, LizardF_getErrorName(results[i]));
            return;
        }
    lzk_err()[0] = 0;
}

/* ---- the readers: the walk of a batch of frames ---- */

/* The count pass.  Frame i is *(const void**)(srcs + i * srcStride), *(const size_t*)(sizes + i * sizeStride) bytes long, and is
 * walked when state[i] is 0.  Stream S starts behind what the caller's stream holds; the frame table goes up, every open frame is
 * walked without tables, one LzWalkResult per frame comes down: the first wait of the call. */
static inline int lz_count_pass(LzCtx* c, size_t nFrames, const unsigned char* state, const void* srcs, size_t srcStride, const void* sizes,
                                size_t sizeStride, LzUnframesEntry* h_frames, LzUnframesEntry* d_frames, LzWalkResult* h_walk, LzWalkResult* d_walk,
                                hipStream_t S, hipStream_t stream)
{
    LzStage* s = c->stage;
    size_t i;
    int rc;
    for (i = 0; i < nFrames; i++) {
        LzUnframesEntry* e = &h_frames[i];
        memset(e, 0, sizeof *e);
        if (state[i]) continue;
        e->src = (uint64_t)(uintptr_t)*(const void* const*)((const char*)srcs + i * srcStride);
        e->srcSize = (uint64_t)*(const size_t*)((const char*)sizes + i * sizeStride);
        e->flags = LZU_WALK;
    }
    LZ_HIP(hipEventRecord(s[0].up, stream));
    LZ_HIP(hipStreamWaitEvent(S, s[0].up, 0));
    LZ_HIP(hipMemcpyAsync(d_frames, h_frames, nFrames * sizeof(LzUnframesEntry), hipMemcpyHostToDevice, S));
    if ((rc = lzk_unframes_walk_launch(d_frames, (uint32_t)nFrames, 0, NULL, NULL, d_walk, S))) return rc;
    LZ_HIP(hipMemcpyAsync(h_walk, d_walk, nFrames * sizeof(LzWalkResult), hipMemcpyDeviceToHost, S));
    LZ_HIP(hipEventRecord(s[0].meta, S));
    LZ_HIP(hipEventSynchronize(s[0].meta));
    return 0;
}

/* the fill pass's entry (zeroed) of a frame the count pass accepted, whose records start at `first` in the batch's record tables */
static inline void lz_fill_entry(LzUnframesEntry* e, const void* src, size_t srcSize, size_t first, const LzWalkResult* w)
{
    e->src = (uint64_t)(uintptr_t)src; e->srcSize = (uint64_t)srcSize;
    e->first = (uint64_t)first; e->nRecords = (uint32_t)w->nRecords;
    e->contentSize = w->contentSize; e->frameBytes = w->frameBytes;
    e->maxBlock = (uint32_t)lzgpu_frame_block_size(w->blockSizeID);
    e->flags = LZU_DECODE;
}

/* ---- the compressors: the blocks of all frames as one list, cut into chunks ---- */

typedef struct {
    LzCtx* c;
    size_t nFrames, nBlocks, maxBlock, perChunk, nChunks;
    const uint8_t* base;                                      /* the lowest source address among the frames that have blocks */
    int level, hash;
    /* the tables every chunk works from, in pinned memory and in the same layout in device memory */
    LzFramesEntry *h_frames, *d_frames;
    uint64_t *h_blkOffsets, *d_blkOffsets;
    uint32_t *h_blkSizes, *d_blkSizes, *h_blkFrames, *d_blkFrames;
    hipStream_t A, B, C;
} LzBatch;

/* a chunk's pack launch on stream B: its blocks are [first, first + q) of the list, bs bytes at most each, compressed into s->d_slots */
typedef int (*lz_batch_pack_fn)(void* arg, const LzBatch* b, const LzStage* s, size_t first, size_t q, size_t bs, uint32_t* d_sizes,
                                uint64_t* d_offsets);

static inline size_t lz_batch_chunk(const LzBatch* b) { return b->nBlocks < b->perChunk ? b->nBlocks : b->perChunk; }

/* a stage's device tables (its d_aux): the compressed sizes and the record positions of the chunk it holds */
static inline size_t lz_batch_aux_bytes(size_t P) { return ((4 * P + 7) & ~(size_t)7) + 8 * P; }

/* the slots and tables of the stages the chunks rotate through, and the call's three streams */
static inline int lz_batch_stages(LzBatch* b)
{
    LzCtx* c = b->c;
    const size_t P = lz_batch_chunk(b);
    size_t s;
    int rc;
    for (s = 0; s < LZ_STAGES && s < b->nChunks; s++) {
        if ((rc = lzp_ensure_dev(c, (void**)&c->stage[s].d_slots, &c->stage[s].d_slots_cap, P * lz_bound_slot(b->maxBlock)))) return rc;
        if ((rc = lzp_ensure_dev(c, (void**)&c->stage[s].d_aux, &c->stage[s].d_aux_cap, lz_batch_aux_bytes(P)))) return rc;
    }
    b->A = c->stage[0].stream; b->B = c->stage[1].stream; b->C = c->stage[2].stream;
    return 0;
}

/* the per-block tables (8 + 4 + 4 bytes per block) start at offset `at` of the call's tables: the offset behind them */
static inline size_t lz_batch_tables_end(const LzBatch* b, size_t at) { return (at + 16 * b->nBlocks + 7) & ~(size_t)7; }

/* ... in the pinned (h) and the device (d) copy of the call's tables */
static inline void lz_batch_block_tables(LzBatch* b, uint8_t* h, uint8_t* d, size_t at)
{
    const size_t T = b->nBlocks, oSizes = at + 8 * T, oFrames = oSizes + 4 * T;
    b->h_blkOffsets = (uint64_t*)(h + at);     b->d_blkOffsets = (uint64_t*)(d + at);
    b->h_blkSizes = (uint32_t*)(h + oSizes);   b->d_blkSizes = (uint32_t*)(d + oSizes);
    b->h_blkFrames = (uint32_t*)(h + oFrames); b->d_blkFrames = (uint32_t*)(d + oFrames);
}

/* the nb blocks of frame i, bs bytes each but the last, behind the *at blocks of the frames before it */
static inline void lz_batch_blocks(LzBatch* b, size_t* at, size_t i, const void* src, size_t srcSize, size_t bs, size_t nb)
{
    size_t k;
    for (k = 0; k < nb; k++, (*at)++) {
        b->h_blkOffsets[*at] = (uint64_t)((const uint8_t*)src + k * bs - b->base);
        b->h_blkSizes[*at] = (uint32_t)(k + 1 == nb ? srcSize - k * bs : bs);
        b->h_blkFrames[*at] = (uint32_t)i;
    }
}

/* stream B starts behind what the caller's stream holds and uploads the tables; A and C start behind the upload */
static inline int lz_batch_upload(LzBatch* b, void* d_tables, const void* h_tables, size_t bytes, hipStream_t stream)
{
    LzStage* s = b->c->stage;
    LZ_HIP(hipEventRecord(s[0].up, stream));
    LZ_HIP(hipStreamWaitEvent(b->B, s[0].up, 0));
    LZ_HIP(hipMemcpyAsync(d_tables, h_tables, bytes, hipMemcpyHostToDevice, b->B));
    LZ_HIP(hipEventRecord(s[1].up, b->B));
    LZ_HIP(hipStreamWaitEvent(b->A, s[1].up, 0));
    LZ_HIP(hipStreamWaitEvent(b->C, s[1].up, 0));
    return 0;
}

/* The hash of every source on C, then every chunk: the block kernels on A into the stage k % LZ_STAGES, `pack` on B behind them;
 * at the end B waits for the hash.  Enqueued, nothing waited for.  *chunks counts the chunks that were packed; *launched (may be
 * NULL) is set once anything was launched. */
static inline int lz_batch_rotate(LzBatch* b, lz_batch_pack_fn pack, void* arg, unsigned long long* chunks, int* launched)
{
    LzCtx* c = b->c;
    const size_t P = lz_batch_chunk(b);
    size_t k;
    int rc;
    if (b->hash) {
        if ((rc = lzk_frames_hash_launch(b->d_frames, (uint32_t)b->nFrames, b->C))) return rc;
        if (launched) *launched = 1;
        LZ_HIP(hipEventRecord(c->stage[2].up, b->C));
    }
    for (k = 0; k < b->nChunks; k++) {
        LzStage* s = &c->stage[k % LZ_STAGES];
        const size_t first = k * b->perChunk, q = b->nBlocks - first < b->perChunk ? b->nBlocks - first : b->perChunk;
        uint32_t* const d_sizes = (uint32_t*)s->d_aux;
        uint64_t* const d_offsets = (uint64_t*)(s->d_aux + ((4 * P + 7) & ~(size_t)7));
        size_t bs = 0, i;
        for (i = first; i < first + q; i++) if (b->h_frames[b->h_blkFrames[i]].blockSize > bs) bs = b->h_frames[b->h_blkFrames[i]].blockSize;
        if (k >= LZ_STAGES) LZ_HIP(hipStreamWaitEvent(b->A, s->done, 0));      /* the slots and tables are free once chunk k - 3 is gathered */
        if ((rc = lzk_launch(c, b->base, q, bs, bs, s->d_slots, lz_bound_slot(bs), d_sizes, b->level, b->A, s->k0, s->k1, b->d_blkSizes + first,
                             b->d_blkOffsets + first))) return rc;
        if (launched) *launched = 1;
        LZ_HIP(hipStreamWaitEvent(b->B, s->k1, 0));
        if ((rc = pack(arg, b, s, first, q, bs, d_sizes, d_offsets))) return rc;
        LZ_HIP(hipEventRecord(s->done, b->B));
        (*chunks)++;
    }
    if (b->hash) LZ_HIP(hipStreamWaitEvent(b->B, c->stage[2].up, 0));
    return 0;
}

#endif
