// unframes_kernels.h — device side of LizardGPU_decompressFrames_device / LizardGPU_framesInfo_device (gfx950): MANY frames that lie
// in device memory, walked, decoded, checked and answered in one batch (lizard_unframes_device.c is the host side).
//
// The single-frame entry (lizard_unframe_device.c) walks and decodes one frame in segments and lets the host decide between them.
// Here the frames of a batch sit side by side in a table of LzUnframesEntry, and every step is ONE launch over all of them:
//   lz_unframes_walk_kernel    one wave per frame runs lz_unframe_walk (unframe_walk.h, unchanged) over the whole frame.  Count mode:
//                              no tables, the host learns every frame's record count and header.  Fill mode: frame f writes its
//                              records' payload offsets and words at offs / words + first_f, at most nRecords_f of them.
//   lz_unframes_kernel         persistent grid, one record per wave (lz_unframe_record, unframe_kernels.h, unchanged): record r of frame
//                              f = recFrame[r] decodes in place, to dst_f + (r - first_f) * maxBlock_f, room min(maxBlock_f, cap_f - at);
//                              a slot that starts at or behind cap_f is LZD_ERR.
//   lz_unframes_settle_kernel  one wave per frame over the frame's per-record results: the frame is CLEAN when every record decoded and
//                              every record but the last filled maxBlock_f — then its records lie where they belong and its size is
//                              (n - 1) * maxBlock + the last result.  Anything else is DELEGATE: the host hands that frame to the
//                              single-frame entry.  Lane 0 also writes the length the hash kernel (lz_xxh32_frames_kernel) is to cover:
//                              the size of a clean frame, 0 otherwise, so that the hash never runs over bytes nobody vouches for.
//   lz_unframes_finish_kernel  one lane per frame, behind the hash: a clean frame whose size differs from the header's content size,
//                              or whose stored checksum (LE32 at src + frameBytes - 4, read by bytes: the address is arbitrary) differs
//                              from the hash, becomes DELEGATE; the result record {size, state} is what the host reads.
// The device never answers a refusal itself: the order of the single entry's refusals is the single entry's business.
// Kernel boundaries in stream order are the only synchronisation.  The C part is shared with the host file; the bodies are written
// against lz_wave.h alone (and unframe_walk.h, which is too), so the CPU SIMT emulator of tests/emul runs them unchanged.
#ifndef LZ_UNFRAMES_KERNELS_H
#define LZ_UNFRAMES_KERNELS_H
#include <stdint.h>
#include "unframe_walk.h"

// One frame of the batch.  The host fills everything (first .. frameBytes after the count pass); the device only reads it.
typedef struct LzUnframesEntry {
    uint64_t src, srcSize;              /* the frame (a device address) */
    uint64_t dst, cap;                  /* where it decodes to (a device address), and the room there */
    uint64_t first;                     /* index of its first record in the batch's record tables */
    uint64_t contentSize, frameBytes;   /* the header's content size (0 = none); the frame's length in src */
    uint32_t nRecords, maxBlock;        /* its records; the block size of its header */
    uint32_t flags, reserved;           /* LZU_* */
} LzUnframesEntry;
typedef struct LzUnframesResult { uint64_t size; uint32_t state, reserved; } LzUnframesResult;
#define LZU_WALK      1u                /* the count pass walks it (the host found nothing wrong with the entry) */
#define LZU_DECODE    2u                /* a normal frame whose chain the count pass accepted: fill pass, decode, settle, finish */
#define LZU_VERIFY    4u                /* it carries a content checksum and the caller wants it verified */
#define LZU_DEAD      0u                /* LzUnframesResult::state: not a frame the device part answers */
#define LZU_CLEAN     1u                /*   size is the decoded size, the bytes lie in dst */
#define LZU_DELEGATE  2u                /*   the single-frame entry decides */
#define LZU_NEED_HISTORY 0xFFFFFFFEu    /* per-record results at and above this are no sizes (LZD_NEED_HISTORY, LZD_ERR of lz_unpack.h) */
#define LZU_WALK_WAVES 4                /* waves per workgroup of the walk and settle kernels */

#ifdef __cplusplus

// All lanes of the wave that owns frame e call.  want: LZU_WALK (count mode, offs / words null) or LZU_DECODE (fill mode).
LZ_DEV void lz_unframes_walk(const LzUnframesEntry* e, u32 want, u64* offs, u32* words, LzWalkResult* res)
{
    if (!(lz_uniform(e->flags) & want)) return;
    const u64 first = lz_uniform64(e->first);
    lz_unframe_walk(reinterpret_cast<const u8*>(lz_uniform64(e->src)), lz_uniform64(e->srcSize), 0, ~0ull, lz_uniform(e->nRecords),
                    offs ? offs + first : nullptr, words ? words + first : nullptr, res);
}

// All lanes of the wave that owns frame e call; out: the per-record results of the batch.
LZ_DEV void lz_unframes_settle(const LzUnframesEntry* e, const u32* out, LzUnframesResult* res, u64* hashBytes)
{
    const u32 lane = lz_lane();
    LzUnframesResult r = { 0ull, LZU_DEAD, 0u };
    if (lz_uniform(e->flags) & LZU_DECODE) {
        const u32 n = lz_uniform(e->nRecords), maxBlock = lz_uniform(e->maxBlock);
        const u32* const mine = out + lz_uniform64(e->first);
        u32 bad = 0;
        for (u32 i = lane; i < n; i += 64u) {
            const u32 v = mine[i];
            if (v >= LZU_NEED_HISTORY || (i + 1u < n && v != maxBlock)) bad = 1u;       // failed, needs history, or short in the middle
        }
        const bool clean = lz_ballot(bad != 0u) == 0ull;
        r.state = clean ? LZU_CLEAN : LZU_DELEGATE;
        if (clean && n) r.size = (u64)(n - 1u) * maxBlock + mine[n - 1u];
    }
    if (lane == 0) { *res = r; *hashBytes = r.size; }
}

// One lane per frame.  hash: XXH32 of dst[0 .. size) when the frame is clean and LZU_VERIFY is set.
LZ_DEV void lz_unframes_finish(const LzUnframesEntry* e, u32 hash, LzUnframesResult* res)
{
    LzUnframesResult r = *res;
    if (r.state == LZU_CLEAN) {
        if (e->contentSize && r.size != e->contentSize) r.state = LZU_DELEGATE;
        else if (e->flags & LZU_VERIFY) {
            const u8* const p = reinterpret_cast<const u8*>(e->src) + e->frameBytes - 4u;
            const u32 stored = (u32)lz_ld8_s(p) | ((u32)lz_ld8_s(p + 1) << 8) | ((u32)lz_ld8_s(p + 2) << 16) | ((u32)lz_ld8_s(p + 3) << 24);
            if (stored != hash) r.state = LZU_DELEGATE;
        }
        if (r.state != LZU_CLEAN) r.size = 0;
    }
    *res = r;
}

#ifdef __HIPCC__
#include "lizard_gpu_ctx.h"             // LzFramesEntry: the table lz_xxh32_frames_kernel (lz_frames_pack.h) hashes from

__global__ __launch_bounds__(64 * LZU_WALK_WAVES) void lz_unframes_walk_kernel(const LzUnframesEntry* frames, u32 nFrames, u32 want, u64* offs,
                                                                              u32* words, LzWalkResult* res)
{
    const u32 f = lz_uniform(blockIdx.x * LZU_WALK_WAVES + (threadIdx.x >> 6));
    if (f >= nFrames) return;
    lz_unframes_walk(frames + f, want, offs, words, res + f);
}

#ifdef LZ_WAVES_DEC      // the decode kernel needs lz_kernels.h and unframe_kernels.h in front of this file (tests/unframes_kernels.hip has neither)
struct LzUnframesBatch {
    const LzUnframesEntry* frames; const u64* offs; const u32* words; const u32* recFrame; u32* out; u32 nRecords;
    u8* scratch; u32* counter;
};

// One wave per record on the persistent grid of the decode kernels (lz_decode_grid, lz_kernels.h), like lz_unframe_inplace_kernel.
__global__ __launch_bounds__(64 * LZ_WAVES_DEC) void lz_unframes_kernel(LzUnframesBatch a)
{
    lz_decode_grid(a.counter, a.nRecords, a.scratch, [&](u32 b, u8* stage, u32* ws) {
        const LzUnframesEntry* const e = a.frames + a.recFrame[b];
        const u64 slot = e->maxBlock, cap = e->cap, at = ((u64)b - e->first) * slot;
        u32 r = LZD_ERR;
        if (at < cap) {
            const u64 room = cap - at < slot ? cap - at : slot;                  // (a block size is 256 MiB at most)
            r = lz_unframe_record(reinterpret_cast<const u8*>(e->src) + a.offs[b], a.words[b], reinterpret_cast<u8*>(e->dst) + at, (u32)room,
                                  stage, ws);
        }
        if (lz_lane() == 0) a.out[b] = r;
    });
}
#endif

__global__ __launch_bounds__(64 * LZU_WALK_WAVES) void lz_unframes_settle_kernel(const LzUnframesEntry* frames, u32 nFrames, const u32* out,
                                                                                LzUnframesResult* results, LzFramesEntry* hashTab)
{
    const u32 f = lz_uniform(blockIdx.x * LZU_WALK_WAVES + (threadIdx.x >> 6));
    if (f >= nFrames) return;
    lz_unframes_settle(frames + f, out, results + f, &hashTab[f].srcSize);
}

__global__ __launch_bounds__(256) void lz_unframes_finish_kernel(const LzUnframesEntry* frames, u32 nFrames, const LzFramesEntry* hashTab,
                                                                 LzUnframesResult* results)
{
    const u32 f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nFrames) return;
    lz_unframes_finish(frames + f, hashTab[f].hash, results + f);
}
#endif  /* __HIPCC__ */
#endif  /* __cplusplus */
#endif
