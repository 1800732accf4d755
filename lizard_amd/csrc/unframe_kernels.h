// unframe_kernels.h — device side of LizardGPU_decompressFrame (gfx950): the block records of a Lizard frame, one wave each.
//
// The host walks the frame (LizardGPU_frameIndex: one 4-byte read per record) and hands a chunk of whole records to the
// device: the chunk's bytes as they sit in the frame, and per record the offset of its payload and its LE32 word (bit 31 =
// stored raw, lib/lizard_frame.c:456-469).  Record i decodes into slot i * slotBytes, slotBytes = the frame's maximum block
// size: every record but the last of a frame normally fills its slot, so the slots ARE the decoded bytes, contiguous.
//   stored raw  : copied by the wave, 16 bytes per lane (the payload sits at an arbitrary byte offset: unaligned loads)
//   compressed  : lz_decompress_block_hist (lz_unpack.h).  A block of a linked frame that copies from before its own start
//                 comes back as LZD_NEED_HISTORY; the host decodes it behind the finished output (nothing waits on the device)
// outSizes[i] = decoded size / LZD_NEED_HISTORY / LZD_ERR, packSizes[i] = the bytes of slot i that are valid (0 for the two
// marks): what lz_scan_kernel / lz_gather_kernel (lz_pack.h, LZ_PACK_PAYLOAD) take when a chunk has a short slot in the middle
// and is packed on the device before it crosses PCIe.
// A wave reads payload[0..size) and writes slot[0..cap) only — the guarantees of the block decoder, and a copy bounded by
// min(size, cap).
#pragma once
#include "lz_unpack.h"

// One record.  All lanes call; the result is wave-uniform.
LZ_DEV u32 lz_unframe_record(const u8* payload, u32 word, u8* slot, u32 cap, u8* stage, u32* ws)
{
    const u32 size = word & 0x7FFFFFFFu;
    if (size == 0u || size > cap) return LZD_ERR;               // (the host's walk has refused both; never trusted here)
    if (word & 0x80000000u) {
        const u32 lane = lz_lane();
        const u32 bulk = size & ~15u;
        for (u32 i = lane * 16u; i < bulk; i += 64u * 16u) lz_st128(slot + i, lz_ld128(payload + i));
        for (u32 i = bulk + lane; i < size; i += 64u) slot[i] = payload[i];
        return size;
    }
    return lz_decompress_block_hist(payload, size, slot, cap > 0x7E000000u ? 0x7E000000u : cap, stage, ws);
}

#ifdef __HIPCC__
struct LzUnframeBatch {
    const u8* src; const u64* payloadOffsets; const u32* words;
    u8* slots; u64 slotBytes; u32* outSizes; u32* packSizes; u32 nRecords;
    u8* scratch; u32* counter;
};

// Persistent grid, one wave per record, LDS workspace and scratch slot as lz_decompress_kernel (lz_kernels.h) uses them; like that
// kernel it keeps the loop of lz_decode_grid in its own words (lz_kernels.h says why).
__global__ __launch_bounds__(64 * LZ_WAVES_DEC) void lz_unframe_kernel(LzUnframeBatch a)
{
    __shared__ u32 ws[LZ_WAVES_DEC][LZD_WS_WORDS];
    const u32 wave = lz_uniform(threadIdx.x >> 6);
    u8* stage = a.scratch + ((u64)blockIdx.x * LZ_MAX_WAVES + wave) * LZ_SCRATCH_BYTES;
    const u32 cap = a.slotBytes > 0x7FFFFFFFull ? 0x7FFFFFFFu : (u32)a.slotBytes;
    for (;;) {
        lz_converge();
        const u32 b = lz_claim_index(a.counter);
        if (b >= a.nRecords) break;
        const u32 r = lz_unframe_record(a.src + a.payloadOffsets[b], a.words[b], a.slots + (u64)b * a.slotBytes, cap, stage, ws[wave]);
        if (lz_lane() == 0) { a.outSizes[b] = r; a.packSizes[b] = r >= LZD_NEED_HISTORY ? 0u : r; }
        lz_converge();
    }
}

// The same for a frame decoded where it lies (LizardGPU_decompressFrame_device): the slots are positions inside the caller's buffer.
// Record i goes to dst + i * slotBytes — the place it has when every earlier record fills its block — with room for
// min(slotBytes, dstRoom - i * slotBytes) bytes: the last slot of an exactly-sized buffer is short.  The host launches only records
// whose slot starts inside the buffer (nRecords <= ceil(dstRoom / slotBytes)), so nothing outside dst[0..dstRoom) is written.
struct LzUnframeInPlaceBatch {
    const u8* src; const u64* payloadOffsets; const u32* words;
    u8* dst; u64 slotBytes; u64 dstRoom; u32* outSizes; u32* packSizes; u32 nRecords;
    u8* scratch; u32* counter;
};

__global__ __launch_bounds__(64 * LZ_WAVES_DEC) void lz_unframe_inplace_kernel(LzUnframeInPlaceBatch a)
{
    lz_decode_grid(a.counter, a.nRecords, a.scratch, [&](u32 b, u8* stage, u32* ws) {
        const u64 at = (u64)b * a.slotBytes;
        u32 r = LZD_ERR;
        if (at < a.dstRoom) {
            u64 room = a.dstRoom - at;
            if (room > a.slotBytes) room = a.slotBytes;
            r = lz_unframe_record(a.src + a.payloadOffsets[b], a.words[b], a.dst + at, room > 0x7FFFFFFFull ? 0x7FFFFFFFu : (u32)room, stage, ws);
        }
        if (lz_lane() == 0) { a.outSizes[b] = r; a.packSizes[b] = r >= LZD_NEED_HISTORY ? 0u : r; }
    });
}
#endif
