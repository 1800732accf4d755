/* lizard_gpu_ctx.h — private seam between the host C layer and the HIP side (not installed; the public surface is
 * include/lizard_amd.h).  Plain C: the per-device context the two sides share, and the thin shim the host-buffer pipeline
 * (lizard_pipeline_host.c, C) calls into lizard_gpu.hip (kernel launches, device context).  Everything else the pipeline
 * needs from HIP is the runtime's own C API (hip_runtime_api.h). */
#ifndef LIZARD_GPU_CTX_H
#define LIZARD_GPU_CTX_H
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

#define LZ_STAGES 3                                         /* chunks in flight in the host-buffer pipeline */
#define LZ_MAX_DEVICES 16

/* One stage of the host-buffer pipeline: pinned staging on the host side, input / slot / packed buffers on the device side,
 * its own stream.  The stages alternate so that the copies of one chunk overlap the kernels of another. */
typedef struct LzStage {
    hipStream_t stream;
    hipEvent_t  k0, k1, meta, done, up;                     /* up: the chunk's input is on the device */
    uint8_t*  h_in;     size_t h_in_cap;                    /* pinned */
    uint8_t*  h_out;    size_t h_out_cap;                   /* pinned */
    uint32_t* h_sizes;  uint64_t* h_offsets;  size_t h_meta_cap;   /* pinned, nBlocks (+1) */
    uint8_t*  d_in;     size_t d_in_cap;
    uint8_t*  d_slots;  size_t d_slots_cap;
    uint8_t*  d_packed; size_t d_packed_cap;
    uint32_t* d_sizes;  uint64_t* d_offsets;  size_t d_meta_cap;
    uint8_t*  d_aux;    size_t d_aux_cap;                   /* frame decoding: the chunk's record table and its results (small, like the meta arrays) */
    uint8_t*  h_aux;    size_t h_aux_cap;                   /* pinned */
} LzStage;

/* The combiner of the one-block entry points (Lizard_compress & co, lizard_pipeline_host.c): callers that arrive while a batch
 * is in flight queue up and leave together in the next launch.  Own staging and stream: the members of a batch copy their input
 * into h_in and their output out of h_out themselves, outside the context lock. */
struct LzOneJob;
typedef struct LzCombine {
    pthread_mutex_t mu;
    pthread_cond_t  cv;
    struct LzOneJob *head, *tail;       /* callers waiting for a batch */
    int   busy;                         /* a batch is under way: from the moment its leader takes it until its last member has copied out */
    int   pendingIn, pendingOut;        /* members of the current batch that still have to copy in / out */
    int   queued, lastN, collecting;    /* callers in the queue; members of the previous batch; a leader is waiting for stragglers */
    LzStage st;                         /* staging of the current batch */
    uint32_t* d_srcSizes; uint64_t* d_srcOffsets; uint32_t* h_srcSizes; uint64_t* h_srcOffsets; size_t raggedCap;
    unsigned long long batches, jobs;   /* statistics (LizardGPU_combinerStats) */
    double tLock, tCopyIn, tGpu, tOut;  /* seconds spent by leaders: waiting for the context, members' copy-in, GPU part, until the last member left */
    double tBusySince;
} LzCombine;

/* A scratch arena with its block counter and the per-wave tables of the levels that keep them in global memory.  Every launch
 * needs one to itself.  The context's own (LzCtx::arena[0], made with the context) serves every launch that fills the machine,
 * the hashChain levels and decompression, one after the other; a compress launch SMALLER than the machine that arrives on
 * another stream while that one is busy gets one of up to LZ_ARENAS_MAX - 1 more (allocated on first need, 2.6 GiB + tables
 * each; LIZARDGPU_ARENAS=1..4 caps the total, default 4), so that small launches of different streams run side by side on the
 * CUs they leave each other. */
#define LZ_ARENAS_MAX 4
#define LZ_ARENA_TABLES 2       /* table classes an arena holds: [0] levels 11/31/22/42 (2^18 u32 slots per wave), [1] levels 20/40/21/41 (64 KiB per wave) */
typedef struct LzArena {
    uint8_t* scratch; uint32_t* counter;
    uint8_t* tables[LZ_ARENA_TABLES];       /* allocated on first use */
    size_t   tableSlots[LZ_ARENA_TABLES];   /* per-wave slots behind each (fewer than resident waves under a memory budget) */
    hipEvent_t ev0, ev1;        /* around its last launch */
    hipStream_t lastStream;
    int timed;                  /* ev1 was recorded */
} LzArena;

typedef struct LzCtx {
    int   ready;
    int   device;
    int   cus;
    LzArena arena[LZ_ARENAS_MAX];   /* [0]: the context's own; [1 .. nArenas): the extra ones */
    int   nArenas, maxArenas, nextExtra;
    int      idleLaunches;      /* launches on the context's own arena since an extra arena was last used (they are released after 64) */
    uint8_t* hcSlots;           /* hashChain levels, allocated on first use / when a larger block size arrives */
    size_t   hcMaxBlock, hcNSlots, hcSlotBytes;
    int      hcHasBest;         /* the slots end with the first-search table of levels 16/17/37/38 */
    size_t   devBytes;          /* device memory this context holds in its large buffers (arenas, tables, work areas, staging): what
                                 * LizardGPU_setMemoryBudget bounds and LizardGPU_memoryInUse reports */
    hipEvent_t lastEv0, lastEv1;   /* around the most recent launch, whichever arena it used (LizardGPU_lastKernelMs) */
    int   lastSplit;            /* the last compress launch was the producer / consumer form (profile builds: where the records are) */
    int   laneOrderOk;          /* self-check at context creation: lanes of one DS atomic are served in lane order */
    float hostKernelMs;         /* sum over the chunks of the last host-buffer call (< 0: last call was a device call) */
    unsigned long long unframeStats[5];   /* LizardGPU_frameDecodeStats [0..3], [4] = chunks packed on the device; since process start */
    /* LizardGPU_decompressFrame_device / LizardGPU_frameIndex_device (lizard_unframe_device.c): the record tables, per-record results
     * and result records of the two walk segments in flight (device, counted in devBytes) and its statistics; its staging slots and
     * pinned buffers are the stages'.  LizardGPU_compressFrames_device (lizard_frames_device.c) keeps the tables of a call here too, and so
     * does LizardGPU_decompressFrames_device (lizard_unframes_device.c). */
    uint8_t* dfTab;     size_t dfTabCap;
    unsigned long long devFrameStats[4];  /* LizardGPU_frameDecodeDeviceStats; since process start */
    unsigned long long devFrameCompressStats[4];   /* LizardGPU_frameCompressDeviceStats (lizard_frame_device.c); since process start */
    unsigned long long devFramesDecodeStats[4];    /* LizardGPU_framesDecodeDeviceStats (lizard_unframes_device.c); since process start */
    unsigned long long devStreamDecodeStats[4];    /* LizardGPU_streamDecodeDeviceStats (lizard_unstream_device.c); since process start */
    unsigned long long devStreamCompressStats[4];  /* LizardGPU_streamCompressDeviceStats (lizard_stream_device.c); since process start */
    unsigned long long devPlanesStats[4];          /* LizardGPU_planesStats (lizard_planes_device.c); since process start */
    unsigned long long devBitPlanesStats[4];       /* LizardGPU_bitPlanesStats (lizard_planes_device.c); since process start */
    unsigned long long devPlanesXorStats[4];       /* LizardGPU_planesXorStats (lizard_planes_device.c); since process start */
    unsigned long long devSeekStats[4];            /* LizardGPU_seekDeviceStats (lizard_seek_device.c); since process start */
    unsigned long long devSliceStats[4];           /* LizardGPU_sliceDeviceStats (lizard_slice_device.c); since process start */
    LzStage stage[LZ_STAGES];
    LzCombine comb;
    pthread_mutex_t mu;
} LzCtx;

/* Locks the selected device's context and makes that device current for the calling thread (HIP's current device is per
 * thread); release restores the caller's device.  rc != 0: nothing is held (the error text is set). */
typedef struct LzGuard { LzCtx* c; int saved; int rc; } LzGuard;

#ifdef __cplusplus
extern "C" {
#endif
void  lzk_guard_acquire(LzGuard* g);
void  lzk_guard_release(LzGuard* g);
char* lzk_err(void);                                        /* the calling thread's error text, LZK_ERR_BYTES bytes */
#define LZK_ERR_BYTES 256
int   lzk_ctx_init(LzCtx* c);
/* device memory of the context's large buffers: counted against the memory budget (-LIZARDGPU_ERR_NOMEM when it does not fit) */
int   lzk_dev_alloc(LzCtx* c, void** p, size_t bytes);
void  lzk_dev_free(LzCtx* c, void* p, size_t bytes);
size_t lzk_budget(void);                                    /* 0 = none */
size_t lzk_budget_room_for_staging(const LzCtx* c);         /* (size_t)-1 = no budget; else what the budget leaves beside the context's scratch arena */
int   lzk_clamp_level(int level);
/* the block kernels over nBlocks blocks resident at d_src (launcher of LizardGPU_compressBlocks_device); k0 / k1 (may be NULL)
 * are recorded around the kernel; d_srcSizes / d_srcOffsets (may be NULL): a ragged batch, block b = d_srcSizes[b] bytes at d_src + d_srcOffsets[b] */
int   lzk_launch(LzCtx* c, const void* d_src, size_t nBlocks, size_t blockSize, size_t lastBlockSize, void* d_dst, size_t dstStride,
                 uint32_t* d_sizes, int level, hipStream_t stream, hipEvent_t k0, hipEvent_t k1, const uint32_t* d_srcSizes,
                 const uint64_t* d_srcOffsets);
/* the calling thread's selected device's context WITHOUT locking it (NULL: no device, the error text is set) */
LzCtx* lzk_ctx_peek(void);
/* lizard_pipeline_host.c: release the combiner's buffers (context locked, no batch under way); keep batches out during a shutdown */
void  lzk_combiner_free(LzCtx* c);
void  lzk_combiner_quiesce(LzCtx* c);
void  lzk_combiner_resume(LzCtx* c);
int   lzk_launch_decompress(LzCtx* c, const void* d_src, const uint64_t* d_offsets, size_t srcStride, const uint32_t* d_srcSizes,
                            size_t nBlocks, void* d_dst, size_t dstStride, uint32_t* d_outSizes, hipStream_t stream);
/* the block records of one chunk of a frame (unframe_kernels.h): record i = word d_words[i], payload at d_src + d_payloadOffsets[i],
 * decoded into slot i * slotBytes; d_outSizes[i] = size / 0xFFFFFFFE (needs history) / 0xFFFFFFFF, d_packSizes[i] = valid bytes of the slot */
int   lzk_launch_unframe(LzCtx* c, const void* d_src, const uint64_t* d_payloadOffsets, const uint32_t* d_words, size_t nRecords, void* d_slots,
                         size_t slotBytes, uint32_t* d_outSizes, uint32_t* d_packSizes, hipStream_t stream);
/* one segment of the walk over the frame at d_src (unframe_walk.h): from startPos (0 = the header first) over at most `budget`
 * records; the first tableCap of them go to d_offs / d_words (either may be NULL); *d_res tells how the segment ended */
struct LzWalkResult;
int   lzk_launch_walk(LzCtx* c, const void* d_src, size_t srcSize, size_t startPos, size_t budget, size_t tableCap, uint64_t* d_offs,
                      uint32_t* d_words, struct LzWalkResult* d_res, hipStream_t stream);
/* lzk_launch_unframe with the slots inside the caller's buffer: record i decodes to d_dst + i * slotBytes, room
 * min(slotBytes, dstRoom - i * slotBytes); nRecords <= ceil(dstRoom / slotBytes) */
int   lzk_launch_unframe_inplace(LzCtx* c, const void* d_src, const uint64_t* d_payloadOffsets, const uint32_t* d_words, size_t nRecords,
                                 void* d_dst, size_t slotBytes, size_t dstRoom, uint32_t* d_outSizes, uint32_t* d_packSizes, hipStream_t stream);
/* exclusive scan of the record sizes + compaction of the valid bytes into d_packed (lz_pack.h); mode: LZK_PACK_* */
void  lzk_pack_launch(const void* d_in, const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, void* d_packed,
                      uint32_t nb, uint32_t blockSize, uint32_t lastBlockSize, int mode, hipStream_t stream);
/* one chunk of a frame assembled in device memory (lz_frame_pack.h): the frame records of nb blocks — slots as lzk_launch left them,
 * raw input at d_in — go to d_dst + (the cursor of *d_state + their prefix sum); the cursor advances, the overflow flag of *d_state
 * rises when it passes `limit`, and no record that ends behind `limit` is written.  d_state: 4 x uint64 in device memory
 * (cursor, overflow, raw records, reserved) */
int   lzk_frame_pack_launch(const void* d_in, const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, void* d_dst,
                            uint32_t nb, uint32_t blockSize, uint32_t lastBlockSize, uint64_t* d_state, uint64_t limit, hipStream_t stream);
/* LizardGPU_compressFrames_device (lizard_frames_device.c, lz_frames_pack.h): one entry per frame of the batch, in device memory for
 * the whole call.  The host fills everything; the device advances cursor, raises overflow, counts rawRecords and sets hash. */
typedef struct LzFramesEntry {
    uint64_t dst, limit;                /* the frame's place (a device address); capacity minus end mark and checksum */
    uint64_t cursor;                    /* where the next record goes: starts at headerBytes */
    uint64_t src, srcSize;              /* what the checksum covers (a device address) */
    uint32_t overflow, rawRecords;      /* sticky: the cursor passed the limit; blocks stored raw so far */
    uint32_t blockSize, nBlocks;        /* (the host's own notes: the kernels find a frame's blocks through the per-block frame index) */
    uint32_t hash, headerBytes, flags;  /* LZK_FRAMES_* */
    uint8_t  header[20];                /* lzgpu_frame_write_header's bytes (at most 15) */
} LzFramesEntry;
typedef struct LzFramesResult { uint64_t size; uint32_t rawRecords, reserved; } LzFramesResult;   /* size: the frame's, or LZK_FRAMES_OVERFLOW */
#define LZK_FRAMES_LIVE      1u         /* not refused by the host: the kernels leave every other entry and its d_dst alone */
#define LZK_FRAMES_CHECKSUM  2u
#define LZK_FRAMES_OVERFLOW  (~(uint64_t)0)
/* one chunk of the batch (lz_frames_pack.h): block b of the chunk is d_blkSizes[b] bytes at d_base + d_blkOffsets[b] and belongs to
 * frame d_blkFrames[b] (blocks of one frame are neighbours); its record — slot b as lzk_launch left it, or that input — goes to
 * the frame's dst + (the frame's cursor + the record bytes of the frame's earlier blocks in this chunk), written to d_offsets[b];
 * cursors advance, and no record that ends behind its frame's limit is written */
int   lzk_frames_pack_launch(const void* d_base, const uint64_t* d_blkOffsets, const uint32_t* d_blkSizes, const uint32_t* d_blkFrames,
                             const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, uint32_t nb,
                             LzFramesEntry* d_frames, hipStream_t stream);
/* XXH32 (seed 0) of every live entry's source that asks for a checksum -> its hash */
int   lzk_frames_hash_launch(LzFramesEntry* d_frames, uint32_t nFrames, hipStream_t stream);
/* header, end mark and checksum of every live entry, and every entry's result record */
int   lzk_frames_finish_launch(const LzFramesEntry* d_frames, LzFramesResult* d_results, uint32_t nFrames, hipStream_t stream);
/* LizardGPU_compressStream_device (lizard_stream_device.c, lz_stream_pack.h): many frames, ONE destination.  The frames' LzFramesEntry
 * table (every entry names d_dst, limit = dstCapacity; the hash and the gather kernel of lz_frames_pack.h work from it unchanged)
 * has a twin with what only a stream needs.  A frame's position is `fixed` + the record bytes of all blocks in front of it, and
 * only the device knows the second term: the scan that meets the frame's first block writes it to `before`. */
typedef struct LzStreamEntry {
    uint64_t fixed;                     /* prefixes and headers up to and including this frame's + end marks and checksum words of the frames before it */
    uint64_t before;                    /* DEVICE: record bytes of the blocks in front of this frame's first block (frames with blocks only) */
    uint64_t prefixOff, prefixBytes;    /* this frame's prefix in the blob */
    uint32_t firstBlock, lastBlock;     /* in the list of all blocks; 0xFFFFFFFF: a frame without blocks */
    uint32_t nextSelf, nextAfter;       /* the first frame with blocks at or behind this one / behind this one; nFrames: none, the stream's end */
    uint32_t tailBytes, reserved;       /* end mark (+ checksum word) */
} LzStreamEntry;
typedef struct LzStreamState { uint64_t carry; uint32_t overflow, rawRecords; } LzStreamState;   /* carry: record bytes of the chunks scanned so far */
/* one chunk (the arguments of lzk_frames_pack_launch; firstBlock: the chunk's place in the list of all blocks): record b goes to
 * d_dst + d_offsets[b] = carry + record bytes of the chunk's earlier blocks + its frame's fixed bytes; the carry advances, raw
 * records are counted, the sticky overflow flag rises when a record, or the tail behind a frame's last record, would pass `capacity`,
 * and no record that ends behind `capacity` is written */
int   lzk_stream_pack_launch(const void* d_base, const uint64_t* d_blkOffsets, const uint32_t* d_blkSizes, const uint32_t* d_blkFrames,
                             const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, uint32_t nb, uint32_t firstBlock,
                             const LzFramesEntry* d_frames, LzStreamEntry* d_entries, LzStreamState* d_state, uint64_t capacity, hipStream_t stream);
/* behind the last gather and the hash: every frame's prefix, header, end mark and checksum word, d_offsets[0 .. nFrames] and the
 * result record (size = fixedTotal + carry, or LZK_FRAMES_OVERFLOW, and then nothing else is written) */
int   lzk_stream_finish_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const void* d_blob, const LzStreamState* d_state,
                               uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, LzFramesResult* d_result, uint64_t* d_offsets,
                               hipStream_t stream);
/* LizardGPU_compressSeekableStream_device (lizard_seek_device.c): behind lzk_stream_finish_launch on the same stream, the seek table
 * frame of 24 nFrames + 24 bytes at the end of the stream, whose size fixedTotal already counts; nothing after an overflow */
int   lzk_stream_seektable_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const LzStreamState* d_state,
                                  const uint64_t* d_offsets, uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, hipStream_t stream);
/* LizardGPU_decompressFrames_device (lizard_unframes_device.c, unframes_kernels.h): the four launches over a batch of frames in device
 * memory.  walk: one wave per frame whose flags have LZU_WALK (fill = 0: no tables) or LZU_DECODE (fill = 1: frame f's records go to
 * d_offs / d_words + first_f); d_res[f] tells how frame f's walk ended.  decode: record r of frame d_recFrame[r] in place in that
 * frame's buffer, d_out[r] = size / 0xFFFFFFFE (needs history) / 0xFFFFFFFF.  settle: d_results[f] = clean with its size, or delegate;
 * d_hashTab[f].srcSize = the bytes lz_xxh32_frames_kernel is to hash.  finish: content size and checksum of the clean frames. */
struct LzUnframesEntry;
struct LzUnframesResult;
int   lzk_unframes_walk_launch(const struct LzUnframesEntry* d_frames, uint32_t nFrames, int fill, uint64_t* d_offs, uint32_t* d_words,
                               struct LzWalkResult* d_res, hipStream_t stream);
int   lzk_unframes_decode_launch(LzCtx* c, const struct LzUnframesEntry* d_frames, const uint64_t* d_offs, const uint32_t* d_words,
                                 const uint32_t* d_recFrame, uint32_t* d_out, size_t nRecords, hipStream_t stream);
int   lzk_unframes_settle_launch(const struct LzUnframesEntry* d_frames, uint32_t nFrames, const uint32_t* d_out, struct LzUnframesResult* d_results,
                                 LzFramesEntry* d_hashTab, hipStream_t stream);
int   lzk_unframes_finish_launch(const struct LzUnframesEntry* d_frames, uint32_t nFrames, const LzFramesEntry* d_hashTab,
                                 struct LzUnframesResult* d_results, hipStream_t stream);
/* LizardGPU_decompressStream_device (lizard_unstream_device.c, unstream_kernels.h): one segment of the walk across the frames of the
 * stream at d_src, one wave: from d_ctl->pos, frame after frame, each frame's walk result and stream offset into d_res / d_offs
 * (tableCap entries each), until the stream ends, the table is full or a frame is refused; *d_ctl tells where and why it stopped */
struct LzStreamCtl;
int   lzk_unstream_walk_launch(const void* d_src, size_t srcSize, struct LzStreamCtl* d_ctl, struct LzWalkResult* d_res, uint64_t* d_offs,
                               uint32_t tableCap, hipStream_t stream);
/* LizardGPU_splitPlanes_device / LizardGPU_joinPlanes_device (lizard_planes_device.c, planes_kernels.h) and, with bits != 0,
 * LizardGPU_splitBitPlanes_device / LizardGPU_joinBitPlanes_device (bitplanes_kernels.h): the one launch over the nTiles tiles of the
 * batch's nEntries non-empty buffers, whose table lies at d_tab */
struct LzPlanesEntry;
int   lzk_planes_launch(LzCtx* c, const struct LzPlanesEntry* d_tab, uint32_t nEntries, uint32_t nTiles, int join, int bits, hipStream_t stream);
/* LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device: the same launch over a table of entries with a base each */
struct LzPlanesXorEntry;
int   lzk_planes_xor_launch(LzCtx* c, const struct LzPlanesXorEntry* d_tab, uint32_t nEntries, uint32_t nTiles, int join, int bits, hipStream_t stream);
/* LizardGPU_decompressFrameRanges_device (lizard_slice_device.c, unslice_kernels.h): behind the fill walk of lzk_unframes_walk_launch, pick p
 * = record d_picks[p].rec of frame d_picks[p].frame decoded to d_dst + d_picks[p].dstOff, a slot of that frame's block size;
 * d_out[p] = size / 0xFFFFFFFE (needs history) / 0xFFFFFFFF */
struct LzSlicePick;
int   lzk_unslice_launch(LzCtx* c, const struct LzUnframesEntry* d_frames, const uint64_t* d_offs, const uint32_t* d_words,
                         const struct LzSlicePick* d_picks, void* d_dst, uint32_t* d_out, size_t nPicks, hipStream_t stream);
/* LizardGPU_joinPlanesRange_device (lizard_slice_device.c, planes_range_kernels.h): the one launch over the nTiles tiles of the batch's
 * nEntries non-empty items, whose table lies at d_tab and whose piece addresses lie at d_pieces */
struct LzPlanesRangeEntry;
int   lzk_planes_range_launch(LzCtx* c, const struct LzPlanesRangeEntry* d_tab, uint32_t nEntries, const uint64_t* d_pieces, uint32_t nTiles,
                              hipStream_t stream);
/* lizard_pipeline_host.c: its staging helpers, shared with lizard_unframe_host.c */
int    lzp_ensure_dev(LzCtx* c, void** p, size_t* cap, size_t need);
int    lzp_ensure_pinned(void** p, size_t* cap, size_t need);
void   lzp_par_memcpy(void* dst, const void* src, size_t n);
int    lzp_is_pinned_host(const void* p);
size_t lzp_chunk_bytes(const LzCtx* ctx);
#define LZK_PACK_PAYLOAD 0
#define LZK_PACK_FRAME   1
#ifdef __cplusplus
}
#endif
#endif
