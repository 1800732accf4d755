// lz_frame_pack.h — a frame assembled in the caller's device buffer, chunk after chunk (LizardGPU_compressFrame_device,
// lizard_frame_device.c; gfx950).
//
// lz_pack.h packs ONE batch from offset 0 and tells the host the total.  A frame of several chunks of slots needs more: the records
// of chunk k+1 start where those of chunk k ended, and the host is not to wait for chunk k to learn where that is.  So the position
// is kept ON THE DEVICE:
//   lz_frame_scan_kernel    exclusive prefix sum of the chunk's frame-record sizes (lz_record_bytes(.., LZ_PACK_FRAME)) STARTING AT
//                           the 64-bit cursor of LzFrameState -> absolute byte position of every record in the frame; advances the
//                           cursor by the chunk's total, counts the chunk's raw records, and raises the sticky overflow flag when
//                           the advanced cursor passes `limit` (dstCapacity minus end mark and checksum)
//   lz_frame_gather_kernel  lz_gather_kernel's copy (one workgroup per block, 16 bytes per lane, scalar tail) to dst + offsets[b];
//                           a record whose end lies behind `limit` is skipped whole, so nothing behind the limit is ever written
// The scans of successive chunks run in stream order (one after the other); the kernel boundary is the only synchronisation: no
// workgroup waits for another.
#pragma once
#include "lz_pack.h"

struct LzFrameState { u64 cursor; u64 overflow; u64 rawRecords; u64 reserved; };

// offsets[i] = state->cursor + sum of record sizes of blocks < i.  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void lz_frame_scan_kernel(const u32* sizes, u64* offsets, u32 nBlocks, u32 blockSize, u32 lastBlockSize,
                                                             LzFrameState* state, u64 limit)
{
    __shared__ u64 part[1024];
    __shared__ u32 rawCount;
    const u32 t = threadIdx.x;
    const u32 per = (nBlocks + 1023u) / 1024u;
    const u32 lo = t * per < nBlocks ? t * per : nBlocks, hi = lo + per < nBlocks ? lo + per : nBlocks;
    const u64 base = state->cursor;                             // (read by every thread before the first barrier, written behind the last)
    u64 sum = 0;
    u32 raw = 0;
    if (t == 0) rawCount = 0;
    for (u32 i = lo; i < hi; i++) {
        const u32 n = i == nBlocks - 1u ? lastBlockSize : blockSize, cs = sizes[i];
        sum += lz_record_bytes(n, cs, LZ_PACK_FRAME);
        raw += lz_frame_stored_raw(n, cs) ? 1u : 0u;
    }
    part[t] = sum;
    __syncthreads();
    if (raw) atomicAdd(&rawCount, raw);
    for (u32 d = 1; d < 1024u; d <<= 1) {                       // Hillis-Steele inclusive scan over the per-thread sums
        const u64 v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = base + part[t] - sum;
    for (u32 i = lo; i < hi; i++) {
        offsets[i] = run;
        run += lz_record_bytes(i == nBlocks - 1u ? lastBlockSize : blockSize, sizes[i], LZ_PACK_FRAME);
    }
    if (t == 1023u) {
        const u64 end = base + part[1023];
        state->cursor = end;
        if (end > limit) state->overflow = 1;
        state->rawRecords += rawCount;
    }
}

// src: the chunk's input (block b at src + b * blockSize), what a raw record copies
__global__ __launch_bounds__(256) void lz_frame_gather_kernel(const u8* src, const u8* slots, u64 slotStride, const u32* sizes, const u64* offsets,
                                                              u8* dst, u32 nBlocks, u32 blockSize, u32 lastBlockSize, u64 limit)
{
    const u32 b = blockIdx.x;
    const u32 n = b == nBlocks - 1u ? lastBlockSize : blockSize;
    const u32 cs = sizes[b];
    const bool raw = lz_frame_stored_raw(n, cs);
    const u32 len = raw ? n : cs;
    const u64 at = offsets[b];
    if (at > limit || limit - at < 4ull + len) return;          // the record would end behind the limit
    u8* out = dst + at;
    const u8* from = raw ? src + (u64)b * blockSize : slots + (u64)b * slotStride;
    if (threadIdx.x == 0) {
        const u32 word = raw ? (n | 0x80000000u) : cs;
        out[0] = (u8)word; out[1] = (u8)(word >> 8); out[2] = (u8)(word >> 16); out[3] = (u8)(word >> 24);
    }
    out += 4;
    const u32 bulk = len & ~15u;
    for (u32 i = threadIdx.x * 16u; i < bulk; i += 256u * 16u)
        lz_st128(out + i, lz_ld128(from + i));
    for (u32 i = bulk + threadIdx.x; i < len; i += 256u) out[i] = from[i];
}

static inline void lz_frame_pack_launch(const u8* d_src, const u8* d_slots, size_t slotStride, const u32* d_sizes, u64* d_offsets, u8* d_dst,
                                        u32 nBlocks, u32 blockSize, u32 lastBlockSize, LzFrameState* d_state, u64 limit, hipStream_t stream)
{
    hipLaunchKernelGGL(lz_frame_scan_kernel, dim3(1), dim3(1024), 0, stream, d_sizes, d_offsets, nBlocks, blockSize, lastBlockSize, d_state, limit);
    hipLaunchKernelGGL(lz_frame_gather_kernel, dim3(nBlocks), dim3(256), 0, stream, d_src, d_slots, (u64)slotStride, d_sizes, (const u64*)d_offsets,
                       d_dst, nBlocks, blockSize, lastBlockSize, limit);
}
