/* lizard_device_common.h — what the host C files that drive the device share (lizard_pipeline_host.c, lizard_unframe_host.c and the
 * lizard_*_device.c entries): the HIP-call check, the frame error codes, "nothing of this call stays in flight", and the small
 * rules every entry that works on device memory states the same way.  Private, plain C, macros and static inline functions only:
 * a file takes what it uses, and the harnesses that compile several of these files into one translation unit get one copy. */

/* a HIP call of a function that answers 0 or -LIZARDGPU_ERR_*: a failure names the call in the thread's error text and returns.
 * In front of the include guard: tests/pipeline_fake.c compiles three of these files into one translation unit and undefines the
 * macro between them, as it did when each file had its own; the next file's include defines it again. */
#ifndef LZ_HIP
#define LZ_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            snprintf(lzk_err(), LZK_ERR_BYTES, "%s failed: %s", #call, hipGetErrorString(e_));         \
            return e_ == hipErrorOutOfMemory ? -LIZARDGPU_ERR_NOMEM : -LIZARDGPU_ERR_HIP;              \
        }                                                                                              \
    } while (0)
#endif

#ifndef LIZARD_DEVICE_COMMON_H
#define LIZARD_DEVICE_COMMON_H
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "unframe_walk.h"

#define LZ_FRAME_E(code)  ((size_t)-(long)(LIZARDGPU_FRAME_ERR_##code))

size_t lzgpu_frame_block_size(unsigned blockSizeID);         /* lizard_frame_host.c */
size_t lzgpu_frame_write_header(uint8_t* dst, const LizardF_frameInfo_t* frameInfo);
size_t lzgpu_frame_device_plan(LizardF_preferences_t* prefs, const LizardF_preferences_t* prefsPtr, const void* d_dst, size_t dstCapacity,
                               const void* d_src, size_t srcSize);

/* lizard_stream_device.c: LizardGPU_compressStream_device with extraFixed bytes of room behind the last frame, which `after` (may be
 * NULL) fills by enqueueing work on stream B behind lz_stream_finish_kernel (0 or -LIZARDGPU_ERR_*, which fails the call) */
typedef int (*lzgpu_stream_after_fn)(void* arg, const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const LzStreamState* d_state,
                                     const uint64_t* d_offsets, uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, hipStream_t B);
size_t lzgpu_stream_compress(void* d_dst, size_t dstCapacity, size_t nFrames, const void* const* d_srcs, const size_t* srcSizes,
                             const void* const* prefixes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs, uint64_t* frameOffsets,
                             size_t* failedFrame, void* stream, uint64_t extraFixed, lzgpu_stream_after_fn after, void* afterArg);

/* the thread's error text across calls that may overwrite it: keep is LZK_ERR_BYTES bytes of the caller's */
static inline void lz_err_save(char* keep) { memcpy(keep, lzk_err(), LZK_ERR_BYTES); }
static inline void lz_err_restore(const char* keep) { memcpy(lzk_err(), keep, LZK_ERR_BYTES); }

/* nothing of this call stays in flight on the stages' streams; the error text survives */
static inline void lz_quiesce(LzCtx* c)
{
    char keep[LZK_ERR_BYTES];
    int i;
    lz_err_save(keep);
    for (i = 0; i < LZ_STAGES; i++) if (c->stage[i].stream) (void)hipStreamSynchronize(c->stage[i].stream);
    (void)hipGetLastError();
    lz_err_restore(keep);
}

/* nothing of a call that failed on the caller's stream stays in flight there; the error text survives */
static inline void lz_drain_caller(hipStream_t stream)
{
    char keep[LZK_ERR_BYTES];
    lz_err_save(keep);
    (void)hipStreamSynchronize(stream);
    (void)hipGetLastError();
    lz_err_restore(keep);
}

/* a table call on the caller's stream: `bytes` of tab go up from pinned memory (stage 0's h_aux) to LzCtx::dfTab, enqueued on stream */
static inline int lz_table_upload(LzCtx* c, const void* tab, size_t bytes, hipStream_t stream)
{
    LzStage* s = c->stage;
    int rc;
    if ((rc = lzk_ctx_init(c))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&s[0].h_aux, &s[0].h_aux_cap, bytes))) return rc;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, bytes))) return rc;
    memcpy(s[0].h_aux, tab, bytes);
    c->hostKernelMs = -1.0f;
    LZ_HIP(hipMemcpyAsync(c->dfTab, s[0].h_aux, bytes, hipMemcpyHostToDevice, stream));
    return 0;
}

/* the streams A, B and C of a call start behind what the caller's stream holds */
static inline int lz_order_after(LzCtx* c, hipStream_t stream, hipStream_t A, hipStream_t B, hipStream_t C)
{
    LZ_HIP(hipEventRecord(c->stage[0].up, stream));
    LZ_HIP(hipStreamWaitEvent(A, c->stage[0].up, 0));
    LZ_HIP(hipStreamWaitEvent(B, c->stage[0].up, 0));
    LZ_HIP(hipStreamWaitEvent(C, c->stage[0].up, 0));
    return 0;
}

/* what a walk (unframe_walk.h) learned from a frame's header */
static inline void lz_walk_info(LizardGPU_frameInfo_t* info, const LzWalkResult* r)
{
    memset(info, 0, sizeof *info);
    info->frameType = (LizardF_frameType_t)r->frameType;
    info->contentSize = r->contentSize;
    if (!r->frameType) {
        info->blockSizeID = (LizardF_blockSizeID_t)r->blockSizeID;
        info->blockMode = (LizardF_blockMode_t)r->blockMode;
        info->contentChecksumFlag = (LizardF_contentChecksum_t)r->checksumFlag;
    }
}

/* the four counters at `offset` in the selected device's context (offsetof(LzCtx, ...Stats)) */
static inline int lz_stats_read(unsigned long long out[4], size_t offset)
{
    LzCtx* c = lzk_ctx_peek();
    if (!out) return -LIZARDGPU_ERR_ARG;
    if (!c) return -LIZARDGPU_ERR_NO_DEVICE;
    pthread_mutex_lock(&c->mu);
    memcpy(out, (const char*)c + offset, 4 * sizeof out[0]);
    pthread_mutex_unlock(&c->mu);
    return 0;
}

/* blocks per chunk of a frame compressed in device memory: LIZARDGPU_FRAME_CHUNK_BLOCKS, or what lzp_chunk_bytes holds */
static inline size_t lz_frame_chunk_blocks(const LzCtx* c, size_t blockSize)
{
    const char* e = getenv("LIZARDGPU_FRAME_CHUNK_BLOCKS");
    const unsigned long v = e && *e ? strtoul(e, NULL, 10) : 0;
    size_t n;
    if (v >= 1 && v <= (1ul << 20)) return (size_t)v;
    n = lzp_chunk_bytes(c) / blockSize;
    return n ? n : 1;
}

/* the slot the block kernels compress one block of blockSize bytes into: its bound, in whole 64-byte lines */
static inline size_t lz_bound_slot(size_t blockSize) { return ((size_t)LIZARD_COMPRESSBOUND((int)blockSize) + 63) & ~(size_t)63; }

#endif
