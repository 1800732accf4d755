// lz_frames_pack.h — many frames assembled in the caller's device buffers from one stream of chunks (LizardGPU_compressFrames_device,
// lizard_frames_device.c; gfx950).
//
// lz_frame_pack.h carries ONE write position in device memory from chunk to chunk.  Here a chunk is a ragged batch of blocks that
// belong to many frames (the blocks of one frame are neighbours, a frame may straddle chunks), and every frame has its own
// destination, limit and cursor in a table of LzFramesEntry (lizard_gpu_ctx.h):
//   lz_frames_scan_kernel    SEGMENTED exclusive prefix sum of the chunk's frame-record sizes: the sum restarts where the per-block frame
//                            index changes -> position of every record inside its own frame's destination = the frame's cursor + the
//                            record bytes of the frame's earlier blocks in this chunk.  Advances the cursor of every frame the chunk
//                            touches, adds the frame's raw records, raises its sticky overflow flag when the cursor passes its limit.
//   lz_frames_gather_kernel  lz_frame_gather_kernel's copy (one workgroup per block, 16 bytes per lane, scalar tail) to the block's
//                            frame's dst + offsets[b]; a record that would end behind that frame's limit is skipped whole.
//   lz_xxh32_frames_kernel   XXH32 (seed 0) of every frame's source.  The four accumulators of one hash are four serial chains and the
//                            stripes of one frame cannot be spread further: four lanes per frame, one accumulator each, sixteen frames
//                            per wave, one wave per workgroup.  The parallelism is ACROSS frames; one frame is hashed at one chain's
//                            pace (not measured yet), whatever the batch holds beside it.
//   lz_frames_finish_kernel  one lane per frame, behind the last gather and the hash: header bytes, end mark, checksum word, result record.
// The rule of lz_frame_pack.h stays: the scans of successive chunks run in stream order, kernel boundaries (and the host's events)
// are the only synchronisation, no workgroup waits for another.
#pragma once
#include "lz_frame_pack.h"
#include "lizard_gpu_ctx.h"

// One workgroup of 1024 threads; thread t owns the blocks [lo, hi).  What a range contributes to the blocks behind it: the record
// bytes and raw records since the last frame border in it, and whether it holds a border at all.
__global__ __launch_bounds__(1024) void lz_frames_scan_kernel(const u32* sizes, const u32* blkSizes, const u32* blkFrames, u64* offsets,
                                                              u32 nBlocks, LzFramesEntry* frames)
{
    __shared__ u64 partBytes[1024];
    __shared__ u32 partRaw[1024];
    __shared__ u32 partBorder[1024];
    const u32 t = threadIdx.x;
    const u32 per = (nBlocks + 1023u) / 1024u;
    const u32 lo = t * per < nBlocks ? t * per : nBlocks, hi = lo + per < nBlocks ? lo + per : nBlocks;
    u64 sum = 0;
    u32 raw = 0, border = 0;
    for (u32 i = lo; i < hi; i++) {
        if (i == 0u || blkFrames[i] != blkFrames[i - 1u]) { sum = 0; raw = 0; border = 1u; }
        sum += lz_record_bytes(blkSizes[i], sizes[i], LZ_PACK_FRAME);
        raw += lz_frame_stored_raw(blkSizes[i], sizes[i]) ? 1u : 0u;
    }
    partBytes[t] = sum; partRaw[t] = raw; partBorder[t] = border;
    __syncthreads();
    for (u32 d = 1; d < 1024u; d <<= 1) {                       // Hillis-Steele inclusive scan; a range with a border forgets what lies in front of it
        const bool take = t >= d && !partBorder[t];
        const u64 vb = take ? partBytes[t - d] : 0ull;
        const u32 vr = take ? partRaw[t - d] : 0u, vf = take ? partBorder[t - d] : 0u;
        __syncthreads();
        if (take) { partBytes[t] += vb; partRaw[t] += vr; partBorder[t] = vf; }
        __syncthreads();
    }
    const u64 carryBytes = t ? partBytes[t - 1u] : 0ull;        // since the border in front of block lo
    const u32 carryRaw = t ? partRaw[t - 1u] : 0u;
    u64 run = carryBytes;
    for (u32 i = lo; i < hi; i++) {
        const u32 f = blkFrames[i];
        if (i == 0u || f != blkFrames[i - 1u]) run = 0;
        offsets[i] = frames[f].cursor + run;
        run += lz_record_bytes(blkSizes[i], sizes[i], LZ_PACK_FRAME);
    }
    __syncthreads();                                            // every cursor has been read: now the thread that owns a frame's last block of the chunk advances it
    run = carryBytes; raw = carryRaw;
    for (u32 i = lo; i < hi; i++) {
        const u32 f = blkFrames[i];
        if (i == 0u || f != blkFrames[i - 1u]) { run = 0; raw = 0; }
        run += lz_record_bytes(blkSizes[i], sizes[i], LZ_PACK_FRAME);
        raw += lz_frame_stored_raw(blkSizes[i], sizes[i]) ? 1u : 0u;
        if (i == nBlocks - 1u || blkFrames[i + 1u] != f) {
            const u64 end = frames[f].cursor + run;
            frames[f].cursor = end;
            if (end > frames[f].limit) frames[f].overflow = 1u;
            frames[f].rawRecords += raw;
        }
    }
}

// base + blkOffsets[b]: the block's input, what a raw record copies
__global__ __launch_bounds__(256) void lz_frames_gather_kernel(const u8* base, const u64* blkOffsets, const u32* blkSizes, const u32* blkFrames,
                                                               const u8* slots, u64 slotStride, const u32* sizes, const u64* offsets,
                                                               const LzFramesEntry* frames)
{
    const u32 b = blockIdx.x;
    const u32 n = blkSizes[b];
    const u32 cs = sizes[b];
    const LzFramesEntry* const f = frames + blkFrames[b];
    const bool raw = lz_frame_stored_raw(n, cs);
    const u32 len = raw ? n : cs;
    const u64 at = offsets[b], limit = f->limit;
    if (at > limit || limit - at < 4ull + len) return;          // the record would end behind its frame's limit
    u8* out = reinterpret_cast<u8*>(f->dst) + at;
    const u8* from = raw ? base + blkOffsets[b] : slots + (u64)b * slotStride;
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

#define LZ_XXH_P1 2654435761u
#define LZ_XXH_P2 2246822519u
#define LZ_XXH_P3 3266489917u
#define LZ_XXH_P4 668265263u
#define LZ_XXH_P5 374761393u
LZ_DEV u32 lz_rotl32(u32 x, u32 r) { return (x << r) | (x >> (32u - r)); }                   // 0 < r < 32
LZ_DEV u32 lz_xxh32_round(u32 acc, u32 w) { return lz_rotl32(acc + w * LZ_XXH_P2, 13u) * LZ_XXH_P1; }

// Lane 4 g + a of a wave holds accumulator a of frame 16 * blockIdx.x + g and reads dword a of every 16-byte stripe (no alignment
// is asked of the source: lz_ld32), eight stripes — one 128-byte line — in flight behind the eight it is mixing in.  Lane 4 g merges
// the four, adds the length, mixes in what is left of the input (below 16 bytes) and writes the frame's hash.
__global__ __launch_bounds__(64) void lz_xxh32_frames_kernel(LzFramesEntry* frames, u32 nFrames)
{
    const u32 a = threadIdx.x & 3u;
    const u32 f = blockIdx.x * 16u + (threadIdx.x >> 2);
    const u32 want = LZK_FRAMES_LIVE | LZK_FRAMES_CHECKSUM;
    const bool active = f < nFrames && (frames[f].flags & want) == want;
    const u8* const p = active ? reinterpret_cast<const u8*>(frames[f].src) : nullptr;
    const u64 n = active ? frames[f].srcSize : 0ull;
    const u64 stripes = n >> 4;
    const u8* const q = p + 4u * a;
    u32 v = a == 0u ? LZ_XXH_P1 + LZ_XXH_P2 : a == 1u ? LZ_XXH_P2 : a == 2u ? 0u : 0u - LZ_XXH_P1;
    u64 s = 0;
    u32 w[8];
    for (u32 k = 0; k < 8u; k++) w[k] = s + 8u <= stripes ? lz_ld32(q + 16u * (s + k)) : 0u;
    while (s + 8u <= stripes) {
        const bool more = s + 16u <= stripes;
        u32 x[8];
#pragma unroll
        for (u32 k = 0; k < 8u; k++) x[k] = more ? lz_ld32(q + 16u * (s + 8u + k)) : 0u;
#pragma unroll
        for (u32 k = 0; k < 8u; k++) v = lz_xxh32_round(v, w[k]);
#pragma unroll
        for (u32 k = 0; k < 8u; k++) w[k] = x[k];
        s += 8u;
    }
    for (; s < stripes; s++) v = lz_xxh32_round(v, lz_ld32(q + 16u * s));
    u32 h = lz_rotl32(v, a == 0u ? 1u : a == 1u ? 7u : a == 2u ? 12u : 18u);
    h += __shfl_xor(h, 1);
    h += __shfl_xor(h, 2);
    if (!active || a != 0u) return;
    if (n < 16ull) h = LZ_XXH_P5;                               // (seed 0)
    h += (u32)n;
    const u8* r = p + (stripes << 4);
    const u8* const end = p + n;
    for (; r + 4 <= end; r += 4) h = lz_rotl32(h + lz_ld32(r) * LZ_XXH_P3, 17u) * LZ_XXH_P4;
    for (; r < end; r++) h = lz_rotl32(h + (u32)*r * LZ_XXH_P5, 11u) * LZ_XXH_P1;
    h ^= h >> 15; h *= LZ_XXH_P2; h ^= h >> 13; h *= LZ_XXH_P3; h ^= h >> 16;
    frames[f].hash = h;
}

// An empty frame is header and tail alone: its cursor never left headerBytes.
__global__ __launch_bounds__(256) void lz_frames_finish_kernel(const LzFramesEntry* frames, LzFramesResult* results, u32 nFrames)
{
    const u32 f = blockIdx.x * 256u + threadIdx.x;
    if (f >= nFrames) return;
    const LzFramesEntry* const e = frames + f;
    LzFramesResult r = { 0ull, 0u, 0u };
    if (e->flags & LZK_FRAMES_LIVE) {
        u8* const dst = reinterpret_cast<u8*>(e->dst);
        const u64 cursor = e->cursor;
        for (u32 i = 0; i < e->headerBytes; i++) dst[i] = e->header[i];
        r.rawRecords = e->rawRecords;
        if (e->overflow || cursor > e->limit) r.size = LZK_FRAMES_OVERFLOW;
        else {                                                  // (the limit leaves room for exactly this)
            u8* const tail = dst + cursor;
            const u32 h = e->hash;
            tail[0] = 0; tail[1] = 0; tail[2] = 0; tail[3] = 0;
            r.size = cursor + 4ull;
            if (e->flags & LZK_FRAMES_CHECKSUM) {
                tail[4] = (u8)h; tail[5] = (u8)(h >> 8); tail[6] = (u8)(h >> 16); tail[7] = (u8)(h >> 24);
                r.size += 4ull;
            }
        }
    }
    results[f] = r;
}

static inline void lz_frames_pack_launch(const u8* d_base, const u64* d_blkOffsets, const u32* d_blkSizes, const u32* d_blkFrames, const u8* d_slots,
                                         size_t slotStride, const u32* d_sizes, u64* d_offsets, u32 nBlocks, LzFramesEntry* d_frames, hipStream_t stream)
{
    hipLaunchKernelGGL(lz_frames_scan_kernel, dim3(1), dim3(1024), 0, stream, d_sizes, d_blkSizes, d_blkFrames, d_offsets, nBlocks, d_frames);
    hipLaunchKernelGGL(lz_frames_gather_kernel, dim3(nBlocks), dim3(256), 0, stream, d_base, d_blkOffsets, d_blkSizes, d_blkFrames, d_slots,
                       (u64)slotStride, d_sizes, (const u64*)d_offsets, (const LzFramesEntry*)d_frames);
}
static inline void lz_frames_hash_launch(LzFramesEntry* d_frames, u32 nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(lz_xxh32_frames_kernel, dim3((nFrames + 15u) / 16u), dim3(64), 0, stream, d_frames, nFrames);
}
static inline void lz_frames_finish_launch(const LzFramesEntry* d_frames, LzFramesResult* d_results, u32 nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(lz_frames_finish_kernel, dim3((nFrames + 255u) / 256u), dim3(256), 0, stream, d_frames, d_results, nFrames);
}
