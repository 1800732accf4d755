// unstream_kernels.h — device side of LizardGPU_decompressStream_device / LizardGPU_streamIndex_device (gfx950): the walk across the
// frame boundaries of a STREAM — frames back to back in one device buffer, no table of pointers — (lizard_unstream_device.c is the
// host side).
//
// The frame behind frame k starts where frame k ends, and where frame k ends is known only once its chain of block records has been
// followed to the end mark: the walk across frames is one serial chain, like the walk inside a frame.  So it is ONE wave:
//   lz_unstream_walk_kernel    starts at the position the control record holds, runs lz_unframe_walk (unframe_walk.h, unchanged, count
//                              mode: no tables) on the frame that starts there, writes that frame's LzWalkResult and its byte offset
//                              in the stream into the frame table, advances by the frame's frameBytes and goes on — until the stream
//                              is used up, the table is full, or the walk refuses a frame (whose status is kept: it is the last
//                              entry).  The control record then holds the frames written, the position reached and why the walk
//                              stopped; the next launch continues from that position, so a stream with more frames than the table
//                              holds is walked in segments.
// No boundary is ever guessed: a magic number inside a payload is payload.
// lz_unframe_walk's lane 0 stores the result record and the whole wave needs two of its words for the next hop: lz_table_sync (the
// ordering point of lz_wave.h for a global-memory word one lane stores and other lanes load) stands between the two, and the words
// are read with lz_ld_shared_u32, which is never served from the scalar cache.
// The C part is shared with the host file; the body is written against lz_wave.h and unframe_walk.h alone, so the CPU SIMT emulator
// of tests/emul runs it unchanged.
#ifndef LZ_UNSTREAM_KERNELS_H
#define LZ_UNSTREAM_KERNELS_H
#include <stdint.h>
#include "unframe_walk.h"

// The control record of a stream walk, in device memory.  The host sets pos (and may leave the rest); a launch reads pos and writes all
// four: pos = the offset of the first frame that is not in the table (of the refused frame when why is LZS_REFUSED), nFrames = entries
// written by THIS launch.
typedef struct LzStreamCtl { uint64_t pos, nFrames; uint32_t why, reserved; } LzStreamCtl;
#define LZS_END      1u                 /* the stream is used up: pos == srcSize */
#define LZS_FULL     2u                 /* the table is full, frames are left */
#define LZS_REFUSED  3u                 /* the walk refused the frame at pos: the last entry holds its status */

#ifdef __cplusplus

// All lanes of one wave call; everything is wave-uniform.  res / offs: the frame table, tableCap (>= 1) entries each.
LZ_DEV void lz_unstream_walk(const u8* src, u64 srcSize, LzStreamCtl* ctl, LzWalkResult* res, u64* offs, u32 tableCap)
{
    const u32 lane = lz_lane();
    u64 pos = lz_uniform64(ctl->pos);
    u32 n = 0, why;
    for (;;) {
        lz_converge();
        if (pos >= srcSize) { why = LZS_END; break; }
        if (n >= tableCap) { why = LZS_FULL; break; }
        LzWalkResult* const r = res + n;
        lz_unframe_walk(src + pos, srcSize - pos, 0, ~0ull, 0, nullptr, nullptr, r);
        if (lane == 0) offs[n] = pos;
        lz_table_sync();                                         // lane 0's record, before any lane reads it
        const u32 status = lz_uniform(lz_ld_shared_u32(&r->status));
        const u32* const fb = reinterpret_cast<const u32*>(&r->frameBytes);
        const u64 frameBytes = (u64)lz_uniform(lz_ld_shared_u32(fb)) | ((u64)lz_uniform(lz_ld_shared_u32(fb + 1)) << 32);
        n++;
        if (status || frameBytes == 0 || frameBytes > srcSize - pos) { why = LZS_REFUSED; break; }   // (an accepted frame is 8 bytes at least and lies inside the stream)
        pos += frameBytes;
    }
    lz_converge();
    if (lane == 0) { ctl->pos = pos; ctl->nFrames = n; ctl->why = why; ctl->reserved = 0; }
}

#ifdef __HIPCC__
__global__ __launch_bounds__(64) void lz_unstream_walk_kernel(const u8* src, u64 srcSize, LzStreamCtl* ctl, LzWalkResult* res, u64* offs, u32 tableCap)
{
    lz_unstream_walk(src, srcSize, ctl, res, offs, tableCap);
}
#endif
#endif  /* __cplusplus */
#endif
