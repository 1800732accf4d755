// planes_kernels.h — device side of LizardGPU_splitPlanes_device / LizardGPU_joinPlanes_device (gfx950): the bytes of a batch of
// buffers regrouped by significance — all byte 0 of every element, then all byte 1, ... (what Blosc calls "shuffle") — and back
// (lizard_planes_device.c is the host side).  A byte-oriented LZ parser and huff0 see the exponent byte of a float only when it
// has a plane of its own.
//
// Layout.  A buffer of `size` bytes with element size E in {1, 2, 4, 8} has n = size / E elements:
//   split   dst[p * n + i] = src[i * E + p]   for p < E, i < n;   the size - n * E tail bytes are copied to dst + n * E
//   join    the exact inverse;   E = 1 is a copy either way.
// Nothing outside dst[0 .. size) is written, nothing outside src[0 .. size) is read.  src and dst may start at any byte address.
//
// Batch.  One launch serves every buffer.  The host cuts each non-empty buffer into TILES of LZP_TILE_BYTES of its elements (the
// last one shorter; a buffer shorter than one element still gets one) and numbers the tiles of the batch through; the device
// table holds one LzPlanesEntry per non-empty buffer, ordered by first tile.  A wave takes tile numbers (a grid stride), finds
// the tile's buffer by bisection of the table — wave-uniform loads — and moves that tile: a thousand 1 MiB buffers fill the device
// as one 1 GiB buffer does.
//
// Lane mapping.  A lane owns 16 consecutive elements: 16 E bytes of the interleaved side, one 16-byte piece of each plane.
//   split   E loads of 16 bytes (the lane's 16 E contiguous bytes), the byte transpose in registers, ONE 16-byte store per plane:
//           every store instruction of the wave is 1 KiB contiguous in its plane.
//   join    one 16-byte load per plane (1 KiB contiguous per instruction), the transpose, E stores of 16 bytes.
// A wave step is 1 024 elements; a tile is 16 / E steps.  The 16-byte accesses (lzp_ld16 / lzp_st16) need no
// alignment (plane p starts at dst + p * n: 16-byte aligned only when n % 16 == 0); they are aligned, and fastest, when the
// buffers are and n % 16 == 0.  Only the last n % 16 elements of a buffer — the ragged end of every plane — and the tail bytes
// move byte by byte, in one lane.
// The transpose is lzp_perm picks (v_perm_b32: any four of the eight bytes of two registers): one per output register for E = 2,
// three for E = 4 and 8 — 0.75 VALU instructions per byte at most, two orders of magnitude below what the memory side delivers.
//
//
// XOR with a base (LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device, lz_planes_xor_tile).  A buffer may come with an
// earlier version of its `size` INTERLEAVED bytes, its base, at any byte address: split writes split(src XOR base), join writes
// join(src) XOR base, every byte taking part (the ragged end and the tail too).  The lane loads from the base the E pieces of 16
// bytes of its interleaved side together with the loads of the step — one memory trip — and XORs in registers: 3 bytes of memory
// traffic per payload byte.  The plain kernels are the XOR = false instantiations of the same bodies and compile to what they were.
//
// The bodies are written against lz_wave.h alone, so the CPU SIMT emulator of tests/emul runs them unchanged (lzp_perm has a
// plain-C form there).
#ifndef PLANES_KERNELS_H
#define PLANES_KERNELS_H
#include <stdint.h>

#define LZP_TILE_BYTES 16384u           /* of a buffer's elements per tile; a multiple of 64 lanes x 16 elements x 8 bytes */

/* One non-empty buffer of the batch, in device memory.  firstTile: the number of its first tile in the batch. */
typedef struct LzPlanesEntry { uint64_t src, dst, size; uint32_t elem, firstTile; } LzPlanesEntry;

/* ... of LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device: split writes dst = split(src XOR base), join writes
 * dst = join(src) XOR base, with `base` an earlier version of the INTERLEAVED bytes, `size` of them, at any byte address.
 * base == 0: this buffer has none and its tiles take the plain path. */
typedef struct LzPlanesXorEntry { uint64_t src, dst, base, size; uint32_t elem, firstTile; } LzPlanesXorEntry;

#ifdef __cplusplus
#include "lz_wave.h"

// Four bytes out of eight: byte k of the result is byte ((sel >> 8 k) & 7) of the 64-bit value hi:lo.
#ifdef __HIPCC__
LZ_DEV u32 lzp_perm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#else
LZ_DEV u32 lzp_perm(u32 hi, u32 lo, u32 sel)
{
    const u64 v = ((u64)hi << 32) | lo;
    u32 r = 0;
    for (u32 k = 0; k < 4; k++) r |= (u32)((v >> (8 * ((sel >> (8 * k)) & 7u))) & 0xFFu) << (8 * k);
    return r;
}
#endif

// The register whose bytes are bytes s0, s1, s2, s3 (byte indices, compile-time after unrolling) of the register array w.
LZ_DEV u32 lzp_pick4(const u32* w, u32 s0, u32 s1, u32 s2, u32 s3)
{
    if ((s0 >> 2) == (s1 >> 2) && (s2 >> 2) == (s3 >> 2))
        return lzp_perm(w[s2 >> 2], w[s0 >> 2], (s0 & 3u) | ((s1 & 3u) << 8) | ((4u + (s2 & 3u)) << 16) | ((4u + (s3 & 3u)) << 24));
    const u32 a = lzp_perm(w[s1 >> 2], w[s0 >> 2], (s0 & 3u) | ((4u + (s1 & 3u)) << 8));
    const u32 b = lzp_perm(w[s3 >> 2], w[s2 >> 2], (s2 & 3u) | ((4u + (s3 & 3u)) << 8));
    return lzp_perm(b, a, 0x05040100u);
}

// 16 elements of E bytes, in registers: interleaved (byte i * E + p) <-> planar (byte p * 16 + i).
template <u32 E, bool JOIN>
LZ_DEV void lzp_transpose16(const u32* in, u32* out)
{
#pragma unroll
    for (u32 m = 0; m < 4 * E; m++) {
        u32 s[4];
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            const u32 o = 4 * m + k;                               // the output byte
            s[k] = JOIN ? (o % E) * 16 + o / E : (o % 16) * E + o / 16;
        }
        out[m] = lzp_pick4(in, s[0], s[1], s[2], s[3]);
    }
}

// The buffers are global memory: on the device the accesses are typed so (global_*, not flat_*: a flat access counts in vmcnt AND
// lgkmcnt), 16 bytes in one instruction at any alignment; on the emulator they are lz_wave.h's, which a test can trace.
#ifdef __HIPCC__
struct __attribute__((packed, aligned(1))) lzp_q128 { u32 w[4]; };
LZ_DEV void lzp_ld16(const u8* p, u32* w) { const LZ_GLOBAL lzp_q128* q = (const LZ_GLOBAL lzp_q128*)p; w[0] = q->w[0]; w[1] = q->w[1]; w[2] = q->w[2]; w[3] = q->w[3]; }
LZ_DEV void lzp_st16(u8* p, const u32* w) { LZ_GLOBAL lzp_q128* q = (LZ_GLOBAL lzp_q128*)p; q->w[0] = w[0]; q->w[1] = w[1]; q->w[2] = w[2]; q->w[3] = w[3]; }
LZ_DEV u32 lzp_ld8(const u8* p) { return *(const LZ_GLOBAL u8*)p; }
LZ_DEV void lzp_st8(u8* p, u32 v) { *(LZ_GLOBAL u8*)p = (u8)v; }
#else
LZ_DEV void lzp_ld16(const u8* p, u32* w) { const lz_u128 v = lz_ld128(p); w[0] = (u32)v.lo; w[1] = (u32)(v.lo >> 32); w[2] = (u32)v.hi; w[3] = (u32)(v.hi >> 32); }
LZ_DEV void lzp_st16(u8* p, const u32* w) { lz_u128 v; v.lo = w[0] | ((u64)w[1] << 32); v.hi = w[2] | ((u64)w[3] << 32); lz_st128(p, v); }
LZ_DEV u32 lzp_ld8(const u8* p) { return lz_ld8_s(p); }
LZ_DEV void lzp_st8(u8* p, u32 v) { lz_st8_s(p, v); }
#endif

// Elements [e0, e1) of a buffer of n elements, e0 a multiple of 1 024: all lanes of one wave call; e0, e1, n are wave-uniform.
// XOR: xb is the buffer's base (LzPlanesXorEntry), the interleaved bytes of an earlier version: the lane loads the 16-byte pieces of
// its 16 E interleaved bytes from xb as well — together with the loads of the step, one memory trip for both — and XORs them in
// registers, before the transpose (split) or behind it (join).
template <u32 E, bool JOIN, bool XOR = false>
LZ_DEV void lzp_move(const u8* src, u8* dst, u64 n, u64 e0, u64 e1, const u8* xb = nullptr)
{
    const u32 lane = lz_lane();
    for (u64 base = e0; base < e1; base += 64 * 16) {
        const u64 i = base + 16 * lane;                            // the lane's first element
        if (i + 16 <= n) {
            u32 in[4 * E], out[4 * E], bx[XOR ? 4 * E : 1];
            if constexpr (E == 1) {
                lzp_ld16(src + i, in);
                if constexpr (XOR) {
                    lzp_ld16(xb + i, bx);
#pragma unroll
                    for (u32 m = 0; m < 4; m++) in[m] ^= bx[m];
                }
                lzp_st16(dst + i, in);
            } else if constexpr (!JOIN) {
#pragma unroll
                for (u32 q = 0; q < E; q++) lzp_ld16(src + i * E + 16 * q, in + 4 * q);
                if constexpr (XOR) {
#pragma unroll
                    for (u32 q = 0; q < E; q++) lzp_ld16(xb + i * E + 16 * q, bx + 4 * q);
#pragma unroll
                    for (u32 m = 0; m < 4 * E; m++) in[m] ^= bx[m];
                }
                lzp_transpose16<E, false>(in, out);
#pragma unroll
                for (u32 p = 0; p < E; p++) lzp_st16(dst + p * n + i, out + 4 * p);
            } else {
#pragma unroll
                for (u32 p = 0; p < E; p++) lzp_ld16(src + p * n + i, in + 4 * p);
                if constexpr (XOR) {
#pragma unroll
                    for (u32 q = 0; q < E; q++) lzp_ld16(xb + i * E + 16 * q, bx + 4 * q);
                }
                lzp_transpose16<E, true>(in, out);
                if constexpr (XOR) {
#pragma unroll
                    for (u32 m = 0; m < 4 * E; m++) out[m] ^= bx[m];
                }
#pragma unroll
                for (u32 q = 0; q < E; q++) lzp_st16(dst + i * E + 16 * q, out + 4 * q);
            }
        } else {
            for (u64 j = i; j < n; j++)                            // the ragged end of the planes: fewer than 16 elements, one lane
                for (u32 p = 0; p < E; p++) {
                    const u32 x = XOR ? lzp_ld8(xb + j * E + p) : 0u;
                    if (!JOIN) lzp_st8(dst + p * n + j, lzp_ld8(src + j * E + p) ^ x);
                    else lzp_st8(dst + j * E + p, lzp_ld8(src + p * n + j) ^ x);
                }
        }
    }
}

// The buffer of tile `tile` (wave-uniform, < the batch's tile count): the last entry whose firstTile <= tile.  Shared with
// bitplanes_kernels.h.
LZ_DEV const LzPlanesEntry* lzp_entry_of(const LzPlanesEntry* tab, u32 nEntries, u32 tile)
{
    u32 lo = 0, hi = nEntries;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (tab[mid].firstTile <= tile) lo = mid; else hi = mid;
    }
    return tab + lo;
}

// Tile t of one buffer: all lanes of one wave call; every argument is wave-uniform.
template <bool JOIN, bool XOR = false>
LZ_DEV void lzp_tile(const u8* src, u8* dst, u64 size, u32 E, u32 t, const u8* xb = nullptr)
{
    const u64 n = size / E;
    const u64 e0 = (u64)t * (LZP_TILE_BYTES / E);
    const u64 e1 = e0 + LZP_TILE_BYTES / E < n ? e0 + LZP_TILE_BYTES / E : n;
    if (E == 2) lzp_move<2, JOIN, XOR>(src, dst, n, e0, e1, xb);
    else if (E == 4) lzp_move<4, JOIN, XOR>(src, dst, n, e0, e1, xb);
    else if (E == 8) lzp_move<8, JOIN, XOR>(src, dst, n, e0, e1, xb);
    else lzp_move<1, JOIN, XOR>(src, dst, n, e0, e1, xb);
    if (t == 0) {                                                  // the bytes behind the last whole element: fewer than E
        const u64 at = n * E + lz_lane();
        if (at < size) lzp_st8(dst + at, lzp_ld8(src + at) ^ (XOR ? lzp_ld8(xb + at) : 0u));
    }
}

// Tile `tile` (< the batch's tile count) of the batch: all lanes of one wave call; everything but the lane's share is wave-uniform.
template <bool JOIN>
LZ_DEV void lz_planes_tile(const LzPlanesEntry* tab, u32 nEntries, u32 tileOfWave)
{
    const u32 tile = lz_uniform(tileOfWave);                       // in SGPRs: the bisection and the entry are scalar loads
    const LzPlanesEntry* const e = lzp_entry_of(tab, nEntries, tile);
    lzp_tile<JOIN>((const u8*)(uintptr_t)e->src, (u8*)(uintptr_t)e->dst, e->size, e->elem, tile - e->firstTile);
}

// ... of a batch with bases: lzp_entry_of for the 40-byte entry, and the tile.  An entry without a base takes the plain path on a
// wave-uniform branch, so a mixed batch is one launch.  Shared with bitplanes_kernels.h.
LZ_DEV const LzPlanesXorEntry* lzp_xor_entry_of(const LzPlanesXorEntry* tab, u32 nEntries, u32 tile)
{
    u32 lo = 0, hi = nEntries;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (tab[mid].firstTile <= tile) lo = mid; else hi = mid;
    }
    return tab + lo;
}

template <bool JOIN>
LZ_DEV void lz_planes_xor_tile(const LzPlanesXorEntry* tab, u32 nEntries, u32 tileOfWave)
{
    const u32 tile = lz_uniform(tileOfWave);
    const LzPlanesXorEntry* const e = lzp_xor_entry_of(tab, nEntries, tile);
    const u8* const src = (const u8*)(uintptr_t)e->src;
    u8* const dst = (u8*)(uintptr_t)e->dst;
    const u8* const xb = (const u8*)(uintptr_t)e->base;
    if (xb) lzp_tile<JOIN, true>(src, dst, e->size, e->elem, tile - e->firstTile, xb);
    else lzp_tile<JOIN>(src, dst, e->size, e->elem, tile - e->firstTile);
}

#ifdef __HIPCC__
#define LZP_WAVES 4                     /* per workgroup */
template <bool JOIN>
LZ_DEV void lz_planes_grid(const LzPlanesEntry* tab, u32 nEntries, u32 nTiles)
{
    const u64 stride = (u64)gridDim.x * LZP_WAVES;
    for (u64 tile = (u64)blockIdx.x * LZP_WAVES + threadIdx.x / 64; tile < nTiles; tile += stride)
        lz_planes_tile<JOIN>(tab, nEntries, (u32)tile);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_planes_split_kernel(const LzPlanesEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_planes_grid<false>(tab, nEntries, nTiles);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_planes_join_kernel(const LzPlanesEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_planes_grid<true>(tab, nEntries, nTiles);
}
template <bool JOIN>
LZ_DEV void lz_planes_xor_grid(const LzPlanesXorEntry* tab, u32 nEntries, u32 nTiles)
{
    const u64 stride = (u64)gridDim.x * LZP_WAVES;
    for (u64 tile = (u64)blockIdx.x * LZP_WAVES + threadIdx.x / 64; tile < nTiles; tile += stride)
        lz_planes_xor_tile<JOIN>(tab, nEntries, (u32)tile);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_planes_xor_split_kernel(const LzPlanesXorEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_planes_xor_grid<false>(tab, nEntries, nTiles);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_planes_xor_join_kernel(const LzPlanesXorEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_planes_xor_grid<true>(tab, nEntries, nTiles);
}
#endif
#endif  /* __cplusplus */
#endif
