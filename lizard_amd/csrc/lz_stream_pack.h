// lz_stream_pack.h — many frames written back to back into ONE device buffer from one stream of chunks
// (LizardGPU_compressStream_device, lizard_stream_device.c; gfx950).
//
// lz_frame_pack.h carries one write position across the chunks of one frame, lz_frames_pack.h one cursor per frame for many
// destinations.  Here frame i starts where frame i - 1 ends.  What of a frame's position does not depend on compressed sizes — the
// prefixes and headers up to its own, the end marks and checksum words of the frames before it — the host knows and puts into the
// table (LzStreamEntry::fixed, lizard_gpu_ctx.h); the rest is the record bytes of ALL blocks in front of it, which only the device
// knows:
//   lz_stream_scan_kernel    PLAIN exclusive prefix sum of the chunk's frame-record sizes on top of ONE carry word in device memory
//                            (LzStreamState::carry) -> position of a record = carry + sum + its frame's fixed bytes.  Notes for every
//                            frame whose first block lies in the chunk the record bytes in front of it (LzStreamEntry::before),
//                            advances the carry, adds the raw records, raises the sticky overflow flag when a record, or the tail
//                            behind a frame's last record, would pass the capacity.
//   the gather               lz_frames_gather_kernel (lz_frames_pack.h) as it is: every LzFramesEntry of the call names d_dst and has
//                            the capacity as its limit, so a record that would end behind it is skipped whole.
//   lz_stream_finish_kernel  one wave per frame, behind the last gather and the hash: prefix bytes, header, end mark and checksum
//                            word at the frame's place, the frame's offset, and (frame 0) the result record.  A frame without blocks
//                            starts where the next frame that has some starts, or at the stream's end.  After an overflow, or when
//                            the total passes the capacity, it writes the result record and nothing else.
//   lz_stream_seektable_kernel  (seekable streams only: LizardGPU_compressSeekableStream_device, lizard_seek_device.c) behind the finish
//                            kernel, one thread per entry: the seek table frame (include/lizard_amd.h Part 3b) in the last
//                            tableBytes bytes of the stream, whose size counts them (they are part of fixedTotal).  Entry i is
//                            { the frame offset the finish kernel wrote, the frame's source size, its prefix bytes, 0 }.  After
//                            an overflow it writes nothing.  Its body, lz_stream_seektable_item, is written against lz_wave.h's
//                            types and the tables of lizard_gpu_ctx.h alone, in front of everything that needs hipcc, so the
//                            CPU SIMT emulator of tests/emul runs it unchanged.
// The rule of lz_frame_pack.h stays: the scans of successive chunks run in stream order, kernel boundaries (and the host's events)
// are the only synchronisation, no workgroup waits for another.
#pragma once
#include "lz_wave.h"
#include "lizard_gpu_ctx.h"

// Byte stores: the table starts wherever the last frame ends.
LZ_DEV void lz_seek_put32(u8* p, u32 v) { p[0] = (u8)v; p[1] = (u8)(v >> 8); p[2] = (u8)(v >> 16); p[3] = (u8)(v >> 24); }
LZ_DEV void lz_seek_put64(u8* p, u64 v) { lz_seek_put32(p, (u32)v); lz_seek_put32(p + 4, (u32)(v >> 32)); }

// Thread i of nFrames + 1: i < nFrames writes entry i, thread nFrames the frame's 8-byte header and the 16-byte footer.
// tableBytes = 24 nFrames + 24; total = fixedTotal + carry is the stream's size, the table its last tableBytes bytes.
LZ_DEV void lz_stream_seektable_item(const LzFramesEntry* frames, const LzStreamEntry* entries, const LzStreamState* state, const u64* offsets,
                                     u32 nFrames, u64 fixedTotal, u64 capacity, u32 i)
{
    const u64 total = fixedTotal + state->carry, tableBytes = 24ull * nFrames + 24ull;
    if (state->overflow != 0u || total > capacity || i > nFrames) return;      // (below: every byte lies in [total - tableBytes, total))
    u8* const table = reinterpret_cast<u8*>(frames[0].dst) + (total - tableBytes);
    if (i < nFrames) {
        u8* const p = table + 8u + 24ull * i;
        lz_seek_put64(p, offsets[i]);
        lz_seek_put64(p + 8, frames[i].srcSize);
        lz_seek_put32(p + 16, (u32)entries[i].prefixBytes);
        lz_seek_put32(p + 20, 0u);
    } else {
        u8* const foot = table + 8u + 24ull * nFrames;
        lz_seek_put32(table, 0x184D2A5Eu);                       // LIZARDGPU_SEEK_MAGIC
        lz_seek_put32(table + 4, (u32)(tableBytes - 8u));
        lz_seek_put64(foot, (u64)nFrames);
        lz_seek_put32(foot + 8, 1u);                             // LIZARDGPU_SEEK_VERSION
        lz_seek_put32(foot + 12, 0x4B535A4Cu);                   // LIZARDGPU_SEEK_TAG "LZSK"
    }
}

#ifdef __HIPCC__
#include "lz_frames_pack.h"

__global__ __launch_bounds__(256) void lz_stream_seektable_kernel(const LzFramesEntry* frames, const LzStreamEntry* entries, const LzStreamState* state,
                                                                  const u64* offsets, u32 nFrames, u64 fixedTotal, u64 capacity)
{
    lz_stream_seektable_item(frames, entries, state, offsets, nFrames, fixedTotal, capacity, blockIdx.x * 256u + threadIdx.x);
}

// One workgroup of 1024 threads; thread t owns the blocks [lo, hi) of the chunk, block firstBlock + i of the call.
__global__ __launch_bounds__(1024) void lz_stream_scan_kernel(const u32* sizes, const u32* blkSizes, const u32* blkFrames, u64* offsets,
                                                              u32 nBlocks, u32 firstBlock, LzStreamEntry* entries, LzStreamState* state,
                                                              u64 capacity)
{
    __shared__ u64 part[1024];
    const u32 t = threadIdx.x;
    const u32 per = (nBlocks + 1023u) / 1024u;
    const u32 lo = t * per < nBlocks ? t * per : nBlocks, hi = lo + per < nBlocks ? lo + per : nBlocks;
    const u64 base = state->carry;                              // (read by every thread before the first barrier, written behind the last)
    u64 sum = 0;
    u32 raw = 0, over = 0;
    for (u32 i = lo; i < hi; i++) {
        sum += lz_record_bytes(blkSizes[i], sizes[i], LZ_PACK_FRAME);
        raw += lz_frame_stored_raw(blkSizes[i], sizes[i]) ? 1u : 0u;
    }
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024u; d <<= 1) {                       // Hillis-Steele inclusive scan over the per-thread sums
        const u64 v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = base + part[t] - sum;                             // record bytes of the call in front of block lo
    for (u32 i = lo; i < hi; i++) {
        LzStreamEntry* const e = entries + blkFrames[i];
        const u32 g = firstBlock + i;
        const u64 fixed = e->fixed;
        if (g == e->firstBlock) e->before = run;
        offsets[i] = fixed + run;
        run += lz_record_bytes(blkSizes[i], sizes[i], LZ_PACK_FRAME);
        if (fixed + run + (g == e->lastBlock ? (u64)e->tailBytes : 0ull) > capacity) over = 1u;
    }
    if (over) state->overflow = 1u;
    if (raw) atomicAdd(&state->rawRecords, raw);
    if (t == 1023u) state->carry = base + part[1023];
}

// One wave per frame.  total = fixedTotal (every prefix, header, end mark and checksum word of the call) + the final carry.
__global__ __launch_bounds__(64) void lz_stream_finish_kernel(const LzFramesEntry* frames, const LzStreamEntry* entries, const u8* blob,
                                                              const LzStreamState* state, u32 nFrames, u64 fixedTotal, u64 capacity,
                                                              LzFramesResult* result, u64* offsets)
{
    const u32 f = blockIdx.x, t = threadIdx.x;
    const u64 carry = state->carry, total = fixedTotal + carry;
    const bool over = state->overflow != 0u || total > capacity;
    if (f == 0u && t == 0u) {
        LzFramesResult r = { over ? LZK_FRAMES_OVERFLOW : total, state->rawRecords, 0u };
        *result = r;
        offsets[nFrames] = total;
    }
    if (over) return;                                           // (below: every byte lies in front of `total`)
    const LzFramesEntry* const e = frames + f;
    const LzStreamEntry* const s = entries + f;
    const u64 before = s->nextSelf < nFrames ? entries[s->nextSelf].before : carry;      // record bytes in front of this frame ...
    const u64 after = s->nextAfter < nFrames ? entries[s->nextAfter].before : carry;     // ... and up to its end
    const u32 headerBytes = e->headerBytes, tailBytes = s->tailBytes, h = e->hash;
    const u64 prefixBytes = s->prefixBytes;
    const u64 start = s->fixed - headerBytes - prefixBytes + before;
    u8* const dst = reinterpret_cast<u8*>(e->dst);
    u8* const head = dst + start;
    const u8* const prefix = blob + s->prefixOff;
    for (u64 i = t; i < prefixBytes; i += 64u) head[i] = prefix[i];
    if (t < headerBytes) head[prefixBytes + t] = e->header[t];
    if (t < tailBytes) dst[s->fixed + after + t] = t < 4u ? (u8)0 : (u8)(h >> (8u * (t - 4u)));
    if (t == 0u) offsets[f] = start;
}

static inline void lz_stream_pack_launch(const u8* d_base, const u64* d_blkOffsets, const u32* d_blkSizes, const u32* d_blkFrames, const u8* d_slots,
                                         size_t slotStride, const u32* d_sizes, u64* d_offsets, u32 nBlocks, u32 firstBlock,
                                         const LzFramesEntry* d_frames, LzStreamEntry* d_entries, LzStreamState* d_state, u64 capacity, hipStream_t stream)
{
    hipLaunchKernelGGL(lz_stream_scan_kernel, dim3(1), dim3(1024), 0, stream, d_sizes, d_blkSizes, d_blkFrames, d_offsets, nBlocks, firstBlock, d_entries,
                       d_state, capacity);
    hipLaunchKernelGGL(lz_frames_gather_kernel, dim3(nBlocks), dim3(256), 0, stream, d_base, d_blkOffsets, d_blkSizes, d_blkFrames, d_slots,
                       (u64)slotStride, d_sizes, (const u64*)d_offsets, d_frames);
}
static inline void lz_stream_finish_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const u8* d_blob, const LzStreamState* d_state,
                                           u32 nFrames, u64 fixedTotal, u64 capacity, LzFramesResult* d_result, u64* d_offsets, hipStream_t stream)
{
    hipLaunchKernelGGL(lz_stream_finish_kernel, dim3(nFrames), dim3(64), 0, stream, d_frames, d_entries, d_blob, d_state, nFrames, fixedTotal, capacity,
                       d_result, d_offsets);
}
static inline void lz_stream_seektable_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const LzStreamState* d_state,
                                              const u64* d_offsets, u32 nFrames, u64 fixedTotal, u64 capacity, hipStream_t stream)
{
    hipLaunchKernelGGL(lz_stream_seektable_kernel, dim3(nFrames / 256u + 1u), dim3(256), 0, stream, d_frames, d_entries, d_state, d_offsets, nFrames,
                       fixedTotal, capacity);
}
#endif  // __HIPCC__
