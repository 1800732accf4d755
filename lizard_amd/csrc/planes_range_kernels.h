// planes_range_kernels.h — device side of LizardGPU_joinPlanesRange_device (gfx950): elements [first, last) of a batch of buffers joined
// out of PIECES of their planes (lizard_slice_device.c is the host side).  A reader that decoded only the blocks that cover a row
// range of a tensor holds, of every plane, the bytes of that range alone, each run somewhere inside a decoded block: a piece is the
// device address of the first byte of one byte range of LizardGPU_planesRangeBytes (lizard_slice_host.c), in that function's order.
//
// Byte planes (planes_kernels.h).  In coordinates relative to `first` the range IS a buffer of last - first elements whose plane p
// starts at piece p: lzr_move is lzp_move<E, true, XOR> with `src + p * n + i` replaced by `piece[p] + i`.  The piece addresses are
// wave-uniform loads; the accesses are 16 bytes per lane at any alignment; the ragged < 16 elements go in one lane.
//
// Bit planes (bitplanes_kernels.h).  The work is done in the tensor's own grid of groups of 8 elements, so no bit ever moves across a
// byte: with f0 = first - first % 8, piece k starts at the plane byte of elements f0 .. f0 + 7, and VIRTUAL element j is element
// f0 + j.  The quads of 128 virtual elements that lie wholly inside [first, min(last, n8)) take lzb_move's join — the quad exchange,
// the 8 x 8 bit transpose, the exchange of pieces — with a plane's address taken from its piece; the partial quads at both edges
// (fewer than 128 + 8 elements at the front, fewer than 128 at the back) go bit by bit, a lane per element byte, and the elements at
// and behind n8, which lie raw in the last piece, byte by byte.  Only elements inside [first, last) are stored.
//
// Batch.  The machinery of planes_kernels.h: tiles of LZP_TILE_BYTES of an item's (virtual) elements numbered through the batch, a
// wave per tile (a grid stride), the item found by bisection of the table with wave-uniform loads.  The table holds one
// LzPlanesRangeEntry per non-empty item, and the piece addresses of the whole batch lie behind it.  Byte and bit items share one
// launch (a wave-uniform branch).  Typed global accesses (lzp_ld16 & co), no LDS, no scratch.
//
// XOR with a base: `base` is the item's base ALREADY ADVANCED to element `first`, (last - first) * E interleaved bytes at any address;
// 0: none, the plain path on a wave-uniform branch.
//
// The bodies are written against lz_wave.h alone, so the CPU SIMT emulator of tests/emul runs them unchanged.
#ifndef PLANES_RANGE_KERNELS_H
#define PLANES_RANGE_KERNELS_H
#include <stdint.h>
#include "bitplanes_kernels.h"

/* One non-empty item of the batch, in device memory.  firstTile: the number of its first tile in the batch; firstPiece: the index of
 * its first piece address in the batch's piece table; filter: 0 = byte planes, 1 = bit planes (LIZARDGPU_FILTER_*). */
typedef struct LzPlanesRangeEntry { uint64_t dst, base, nElems, first, last; uint32_t elem, filter, firstTile, firstPiece; } LzPlanesRangeEntry;

#ifdef __cplusplus

// Byte planes: elements [e0, e1) of a range of n elements (relative to its first), e0 a multiple of 1 024: all lanes of one wave call;
// pp (the range's E piece addresses), e0, e1, n are wave-uniform.
template <u32 E, bool XOR>
LZ_DEV void lzr_move(const u64* pp, u8* dst, u64 n, u64 e0, u64 e1, const u8* xb)
{
    const u32 lane = lz_lane();
    const u8* src[E];
#pragma unroll
    for (u32 p = 0; p < E; p++) src[p] = (const u8*)(uintptr_t)pp[p];
    for (u64 base = e0; base < e1; base += 64 * 16) {
        const u64 i = base + 16 * lane;                            // the lane's first element
        if (i + 16 <= n) {
            u32 in[4 * E], out[4 * E], bx[XOR ? 4 * E : 1];
#pragma unroll
            for (u32 p = 0; p < E; p++) lzp_ld16(src[p] + i, in + 4 * p);
            if constexpr (XOR) {
#pragma unroll
                for (u32 q = 0; q < E; q++) lzp_ld16(xb + i * E + 16 * q, bx + 4 * q);
            }
            if constexpr (E == 1) {
#pragma unroll
                for (u32 m = 0; m < 4; m++) out[m] = in[m];
            } else {
                lzp_transpose16<E, true>(in, out);
            }
            if constexpr (XOR) {
#pragma unroll
                for (u32 m = 0; m < 4 * E; m++) out[m] ^= bx[m];
            }
#pragma unroll
            for (u32 q = 0; q < E; q++) lzp_st16(dst + i * E + 16 * q, out + 4 * q);
        } else {
            for (u64 j = i; j < n; j++)                            // the ragged end of the range: fewer than 16 elements, one lane
                for (u32 p = 0; p < E; p++) lzp_st8(dst + j * E + p, lzp_ld8(src[p] + j) ^ (XOR ? lzp_ld8(xb + j * E + p) : 0u));
        }
    }
}

template <u32 E, bool XOR>
LZ_DEV void lzr_tile(const u64* pp, u8* dst, u64 n, u32 t, const u8* xb)
{
    const u64 e0 = (u64)t * (LZP_TILE_BYTES / E);
    const u64 e1 = e0 + LZP_TILE_BYTES / E < n ? e0 + LZP_TILE_BYTES / E : n;
    lzr_move<E, XOR>(pp, dst, n, e0, e1, xb);
}

// Bit planes: virtual elements [e0, e1), e0 a multiple of 2 048: all lanes of one wave call and stay together (the quad exchange).
// pk: the 8 E piece addresses of the planes; virtual element j is stored at dst + (j - skip) * E (skip = first % 8) and XORed with
// xb + (j - skip) * E.  Only the quads that lie wholly inside [w0, w1) (multiples of 128) touch memory; the others take part with
// zeros.  The body is the join of lzb_move (bitplanes_kernels.h), a plane's address taken from its piece.
template <u32 E, bool XOR>
LZ_DEV void lzbr_move(const u64* pk, u8* dst, u64 skip, u64 w0, u64 w1, u64 e0, u64 e1, const u8* xb)
{
    const u32 lane = lz_lane(), q = lane >> 2, r = lane & 3u;
    constexpr u32 H = E / 2;                                       // groups of four pieces in a lane (the exchange of pieces)
    for (u64 base = e0; base < e1; base += LZB_STEP_ELEMS) {
        const u64 q0 = base + (u64)LZB_QUAD_ELEMS * q;             // the quad's first virtual element
        const bool whole = q0 >= w0 && q0 + LZB_QUAD_ELEMS <= w1;
        u32 in[8 * E];                                             // 16 bytes of 2 E planes
        u32 bx[XOR ? 8 * E : 1];                                   // the base's pieces, in the order of the stores
#pragma unroll
        for (u32 m = 0; m < 8 * E; m++) in[m] = 0;
        if (whole) {
#pragma unroll
            for (u32 m = 0; m < 2 * E; m++) {                      // plane 4 m + r: its piece address out of four wave-uniform ones
                const u64 a0 = pk[4 * m], a1 = pk[4 * m + 1], a2 = pk[4 * m + 2], a3 = pk[4 * m + 3];
                const u64 a = r == 0 ? a0 : r == 1 ? a1 : r == 2 ? a2 : a3;
                lzp_ld16((const u8*)(uintptr_t)a + q0 / 8, in + 4 * m);
            }
            if constexpr (XOR) {
                // where the lane's piece m lies on the interleaved side: its own 32 E bytes, or (E >= 2) piece 4 i + r of the quad's
                const u8* const x = xb + (E >= 2 ? (q0 - skip) * E + 16 * r : (base + LZB_LANE_ELEMS * lane - skip) * E);
#pragma unroll
                for (u32 m = 0; m < 2 * E; m++) lzp_ld16(x + (E >= 2 ? 64 * m : 16 * m), bx + 4 * m);
            }
        }
#pragma unroll
        for (u32 p = 0; p < E; p++) {
            lzb_quad_transpose(in + 8 * p);
            lzb_quad_transpose(in + 8 * p + 4);
            lzb_transpose8(in + 8 * p);
        }
        if constexpr (E == 1) {
#pragma unroll
            for (u32 m = 0; m < 2; m++) {
                u32 out[4];
                lzb_from_planes<E>(in, m, out);
                if (whole) {
                    if constexpr (XOR) {
#pragma unroll
                        for (u32 k = 0; k < 4; k++) out[k] ^= bx[4 * m + k];
                    }
                    lzp_st16(dst + (base + LZB_LANE_ELEMS * lane - skip) * E + 16 * m, out);
                }
            }
        } else {
#pragma unroll
            for (u32 h = 0; h < H; h++) {
                u32 o[4][4], t[4][4];                              // o[c][k]: dword k of the lane's piece 4 h + c
#pragma unroll
                for (u32 c = 0; c < 4; c++) lzb_from_planes<E>(in, 4 * h + c, o[c]);
#pragma unroll
                for (u32 k = 0; k < 4; k++) {
                    u32 a[4] = { o[0][k], o[1][k], o[2][k], o[3][k] };
                    lzb_quad_transpose(a);                         // a[c]: dword k of piece 4 h + r of lane c
#pragma unroll
                    for (u32 c = 0; c < 4; c++) t[c][k] = a[c];
                }
                if (whole) {
                    u8* const dq = dst + (q0 - skip) * E + 16 * r;
                    if constexpr (XOR) {
#pragma unroll
                        for (u32 c = 0; c < 4; c++)
#pragma unroll
                            for (u32 k = 0; k < 4; k++) t[c][k] ^= bx[4 * (c * H + h) + k];
                    }
#pragma unroll
                    for (u32 c = 0; c < 4; c++) lzp_st16(dq + 64 * (c * H + h), t[c]);
                }
            }
        }
    }
}

// Virtual elements [a, b) (fewer than 2^32) bit by bit, a lane per element byte.  No lane waits for another.
template <u32 E, bool XOR>
LZ_DEV void lzbr_slow(const u64* pk, u8* dst, u64 skip, u64 a, u64 b, const u8* xb)
{
    const u32 count = (u32)(b - a) * E;
    for (u32 x = lz_lane(); x < count; x += 64) {
        const u64 j = a + x / E;
        const u32 p = x % E;
        u32 v = 0;
        for (u32 bit = 0; bit < 8; bit++) v |= ((lzp_ld8((const u8*)(uintptr_t)pk[8 * p + bit] + j / 8) >> (u32)(j % 8)) & 1u) << bit;
        const u64 at = (j - skip) * E + p;
        lzp_st8(dst + at, v ^ (XOR ? lzp_ld8(xb + at) : 0u));
    }
}

// Tile t of a bit-plane item: elements [first, last) of a buffer of n; pk: 8 E plane pieces and the raw piece behind them.
template <u32 E, bool XOR>
LZ_DEV void lzbr_tile(const u64* pk, u8* dst, u64 n, u64 first, u64 last, u32 t, const u8* xb)
{
    const u64 n8 = n & ~(u64)7, f0 = first & ~(u64)7, skip = first - f0;
    const u64 top = last < n8 ? last : n8;                         // the transposed elements of the range end here
    const u64 a = skip, b = top > first ? top - f0 : skip;         // ... and are the virtual elements [a, b)
    u64 w0 = skip ? LZB_QUAD_ELEMS : 0, w1 = b & ~(u64)(LZB_QUAD_ELEMS - 1);    // whole quads inside [a, b)
    if (w1 <= w0) w0 = w1 = b;                                     // none: everything goes bit by bit, as the front edge
    const u64 len = last - f0;                                     // virtual elements of the item, the raw ones included
    const u64 e0 = (u64)t * (LZP_TILE_BYTES / E);
    const u64 e1 = e0 + LZP_TILE_BYTES / E < len ? e0 + LZP_TILE_BYTES / E : len;
    lzbr_move<E, XOR>(pk, dst, skip, w0, w1, e0, w1 > w0 ? (e1 < w1 ? e1 : w1) : e0, xb);
    if (t == 0) lzbr_slow<E, XOR>(pk, dst, skip, a, w0, xb);       // the partial quad at the front
    if (e1 == len) {                                               // the item's last tile: the partial quad at the back, the raw elements
        lzbr_slow<E, XOR>(pk, dst, skip, w1, b, xb);
        if (last > n8) {
            const u64 r0 = first > n8 ? first : n8;                // fewer than 8 elements: fewer than 64 bytes
            const u64 x = lz_lane(), at = (r0 - first) * E + x;
            if (x < (last - r0) * E) lzp_st8(dst + at, lzp_ld8((const u8*)(uintptr_t)pk[8 * E] + x) ^ (XOR ? lzp_ld8(xb + at) : 0u));
        }
    }
}

// The item of tile `tile` (wave-uniform, < the batch's tile count): the last entry whose firstTile <= tile.
LZ_DEV const LzPlanesRangeEntry* lzr_entry_of(const LzPlanesRangeEntry* tab, u32 nEntries, u32 tile)
{
    u32 lo = 0, hi = nEntries;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (tab[mid].firstTile <= tile) lo = mid; else hi = mid;
    }
    return tab + lo;
}

template <bool XOR>
LZ_DEV void lzr_item_tile(const LzPlanesRangeEntry* e, const u64* pp, u32 t, const u8* xb)
{
    u8* const dst = (u8*)(uintptr_t)e->dst;
    const u64 n = e->nElems, first = e->first, last = e->last;
    const u32 E = e->elem;
    if (e->filter) {
        if (E == 2) lzbr_tile<2, XOR>(pp, dst, n, first, last, t, xb);
        else if (E == 4) lzbr_tile<4, XOR>(pp, dst, n, first, last, t, xb);
        else if (E == 8) lzbr_tile<8, XOR>(pp, dst, n, first, last, t, xb);
        else lzbr_tile<1, XOR>(pp, dst, n, first, last, t, xb);
    } else {
        if (E == 2) lzr_tile<2, XOR>(pp, dst, last - first, t, xb);
        else if (E == 4) lzr_tile<4, XOR>(pp, dst, last - first, t, xb);
        else if (E == 8) lzr_tile<8, XOR>(pp, dst, last - first, t, xb);
        else lzr_tile<1, XOR>(pp, dst, last - first, t, xb);
    }
}

// Tile `tile` (< the batch's tile count) of the batch: all lanes of one wave call; everything but the lane's share is wave-uniform.
// pieces: the piece addresses of the whole batch.
LZ_DEV void lz_planes_range_tile(const LzPlanesRangeEntry* tab, u32 nEntries, const u64* pieces, u32 tileOfWave)
{
    const u32 tile = lz_uniform(tileOfWave);                       // in SGPRs: the bisection, the entry and the pieces are loads of one address per wave
    const LzPlanesRangeEntry* const e = lzr_entry_of(tab, nEntries, tile);
    const u8* const xb = (const u8*)(uintptr_t)e->base;
    const u64* const pp = pieces + e->firstPiece;
    if (xb) lzr_item_tile<true>(e, pp, tile - e->firstTile, xb);
    else lzr_item_tile<false>(e, pp, tile - e->firstTile, nullptr);
}

#ifdef __HIPCC__
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_planes_range_kernel(const LzPlanesRangeEntry* tab, u32 nEntries, const u64* pieces, u32 nTiles)
{
    const u64 stride = (u64)gridDim.x * LZP_WAVES;
    for (u64 tile = (u64)blockIdx.x * LZP_WAVES + threadIdx.x / 64; tile < nTiles; tile += stride)
        lz_planes_range_tile(tab, nEntries, pieces, (u32)tile);
}
#endif
#endif  /* __cplusplus */
#endif
