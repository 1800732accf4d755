// unslice_kernels.h — device side of LizardGPU_decompressFrameRanges_device (gfx950): of a batch of frames in device memory, only the
// records that cover the byte ranges a caller asks for are decoded (lizard_slice_device.c is the host side).
//
// The frames are walked by lz_unframes_walk_kernel (unframes_kernels.h, unchanged: a count pass, then a fill pass that writes every
// record's payload offset and word at its place in the batch tables).  The host turns the ranges into PICKS — which record of which
// frame, where its slot starts in the one destination, how many bytes it must decode to — and
//   lz_unslice_kernel          persistent grid, one pick per wave (lz_decode_grid, lz_kernels.h), the record decoded by
//                              lz_unframe_record (unframe_kernels.h, unchanged) into a slot of its frame's block size: out[pick] is its
//                              size, or LZD_NEED_HISTORY / LZD_ERR.  The host compares it with what the pick must decode to.
// A slot is maxBlock bytes even for a frame's last, shorter record: the record of a tiny last block is longer than what it decodes to.
// The host has tested the sum of the slots against the destination's capacity before the launch.
#ifndef LZ_UNSLICE_KERNELS_H
#define LZ_UNSLICE_KERNELS_H
#include <stdint.h>
#include "unframes_kernels.h"

// One picked record.  rec: its index in the batch's record tables (the frame's first + its number in the frame).
typedef struct LzSlicePick { uint64_t dstOff; uint32_t rec, frame, want, reserved; } LzSlicePick;

#if defined(__cplusplus) && defined(__HIPCC__) && defined(LZ_WAVES_DEC)
struct LzUnsliceBatch {
    const LzUnframesEntry* frames; const u64* offs; const u32* words; const LzSlicePick* picks; u8* dst; u32* out; u32 nPicks;
    u8* scratch; u32* counter;
};

__global__ __launch_bounds__(64 * LZ_WAVES_DEC) void lz_unslice_kernel(LzUnsliceBatch a)
{
    lz_decode_grid(a.counter, a.nPicks, a.scratch, [&](u32 b, u8* stage, u32* ws) {
        const LzSlicePick* const p = a.picks + b;
        const LzUnframesEntry* const e = a.frames + p->frame;
        const u32 rec = p->rec;
        const u32 r = lz_unframe_record(reinterpret_cast<const u8*>(e->src) + a.offs[rec], a.words[rec], a.dst + p->dstOff, e->maxBlock, stage, ws);
        if (lz_lane() == 0) a.out[b] = r;
    });
}
#endif
#endif
