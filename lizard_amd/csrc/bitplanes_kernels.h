// bitplanes_kernels.h — device side of LizardGPU_splitBitPlanes_device / LizardGPU_joinBitPlanes_device (gfx950): the BITS of a batch
// of buffers regrouped by weight — all bit 0 of every element, then all bit 1, ... (what Blosc and HDF5 call "bitshuffle") — and
// back (lizard_planes_device.c is the host side, shared with the byte planes).  A nearly constant bit plane — the sign-extension
// bits of small integers, the top exponent bits of weights — is a long run, which the LZ parser removes without a Huffman stage.
//
// Layout.  A buffer of `size` bytes with element size E in {1, 2, 4, 8}: n = size / E elements, n8 = n - n % 8 of them are
// transposed, P = n8 / 8 bytes per plane.  Bit k (k < 8 E) of element i is (src[i * E + k / 8] >> (k % 8)) & 1.
//   split   dst[k * P + j] = sum over b < 8 of bit_k(element 8 j + b) << b   for k < 8 E, j < P;
//           the bytes src[n8 * E .. size) — the last n % 8 elements and what lies behind the last whole element — are copied
//   join    the exact inverse;   E = 1 is NOT a copy: eight planes.
// Nothing outside dst[0 .. size) is written, nothing outside src[0 .. size) is read.  src and dst may start at any byte address.
//
// Batch.  The machinery of planes_kernels.h, unchanged: LzPlanesEntry, tiles of LZP_TILE_BYTES of a buffer's elements numbered
// through the batch, a wave per tile (a grid stride), the tile's buffer found by bisection (lzp_entry_of).
//
// Lane mapping.  A lane owns 32 consecutive elements, a wave step is 2 048 elements, a tile is 8 / E steps.
//   split   2 E loads of 16 bytes (the lane's 32 E contiguous bytes; the wave's loads of a step cover 2 048 E contiguous bytes),
//           the transpose in registers into 8 E dwords — one per plane, element j in bit j —, then, four planes at a time, the
//           four lanes of a quad exchange dwords (a 4 x 4 transpose) so that lane r of quad q holds 16 contiguous bytes of plane
//           k0 + r, those of elements 128 q .. 128 q + 127 of the step, and ONE 16-byte store per lane per four planes: every
//           store instruction of the wave writes four runs of 256 contiguous bytes, one in each of four planes.
//   join    the mirror image: 2 E loads of 16 bytes from the planes, the quad exchange, the transpose — and, for E >= 2, one more
//           quad exchange, of 16-byte pieces, so that a store instruction writes runs of 64 contiguous bytes and not 16 bytes of
//           every 32 E (lzb_move) —, 2 E stores of 16 bytes.
// The transpose of 32 elements: per byte position p, eight lzp_perm picks gather byte p of elements g, g + 8, g + 16, g + 24 into
// dword g (0.75 v_perm_b32 per byte at most); then an 8 x 8 BIT transpose across those eight dwords, all four byte columns at
// once, in three stages of masked swaps (4-, 2-, 1-bit) of two instructions per register (a shift and v_bfi_b32): 1.5 per byte.
// The quad exchange is two stages of a DPP quad_perm move and a select per register: 1 per byte.  3.25 VALU instructions per
// payload byte for the split and, with the exchange of pieces, 4.25 for the join, beside the addresses.  No LDS, no scratch.
// Whole quads only take this path: the last n8 % 128 elements of a buffer — up to 15 bytes at the end of every plane — move bit by
// bit (one lane per plane byte, or per element byte), and the bytes behind n8 * E byte by byte, in the buffer's last tile.
// The 16-byte accesses need no alignment (plane k starts at dst + k * P).
//
// XOR with a base (lz_bitplanes_xor_tile; planes_kernels.h has the semantics and the entry): the lane loads from the base the 2 E
// pieces of 16 bytes of the interleaved side that it loads from src (split) or is about to store (join), with the loads of the step.
//
// The bodies are written against lz_wave.h alone, so the CPU SIMT emulator of tests/emul runs them unchanged; the quad exchange
// (lzb_quad_xor1 / lzb_quad_xor2: DPP on the device) has a plain form on lz_shfl there.
#ifndef BITPLANES_KERNELS_H
#define BITPLANES_KERNELS_H
#include "planes_kernels.h"

#define LZB_LANE_ELEMS 32u              /* consecutive elements of a lane: one dword of every plane */
#define LZB_QUAD_ELEMS 128u             /* of a quad: 16 bytes of every plane */
#define LZB_STEP_ELEMS 2048u            /* of a wave; LZP_TILE_BYTES / E is a multiple of it for every E */

#ifdef __cplusplus

// The value of lane (lane ^ 1) / (lane ^ 2): all lanes of the wave call.
#ifdef __HIPCC__
template <int CTRL>
LZ_DEV u32 lzb_quad_perm(u32 v) { return (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, true); }
LZ_DEV u32 lzb_quad_xor1(u32 v) { return lzb_quad_perm<0xB1>(v); }   // quad_perm:[1,0,3,2]
LZ_DEV u32 lzb_quad_xor2(u32 v) { return lzb_quad_perm<0x4E>(v); }   // quad_perm:[2,3,0,1]
#else
LZ_DEV u32 lzb_quad_xor1(u32 v) { return lz_shfl(v, lz_lane() ^ 1u); }
LZ_DEV u32 lzb_quad_xor2(u32 v) { return lz_shfl(v, lz_lane() ^ 2u); }
#endif

// v_bfi_b32: the bits of x where m is set, of y elsewhere.
LZ_DEV u32 lzb_bfi(u32 m, u32 x, u32 y) { return (x & m) | (y & ~m); }

// The bits of a under (m << s) <-> the bits of b under m.
LZ_DEV void lzb_swap(u32& a, u32& b, u32 m, u32 s)
{
    const u32 na = lzb_bfi(m, a, b << s), nb = lzb_bfi(m, a >> s, b);
    a = na; b = nb;
}

// An 8 x 8 bit transpose across eight dwords, in each of their four byte columns: bit 8 c + b of x[g] <-> bit 8 c + g of x[b].
LZ_DEV void lzb_transpose8(u32* x)
{
#pragma unroll
    for (u32 g = 0; g < 4; g++) lzb_swap(x[g], x[g + 4], 0x0F0F0F0Fu, 4);
#pragma unroll
    for (u32 g = 0; g < 8; g += 4) { lzb_swap(x[g], x[g + 2], 0x33333333u, 2); lzb_swap(x[g + 1], x[g + 3], 0x33333333u, 2); }
#pragma unroll
    for (u32 g = 0; g < 8; g += 2) lzb_swap(x[g], x[g + 1], 0x55555555u, 1);
}

// Byte position p of 32 interleaved elements of E bytes (8 E registers) -> its eight planes 8 p .. 8 p + 7, element j in bit j.
template <u32 E>
LZ_DEV void lzb_to_planes(const u32* in, u32 p, u32* x)
{
#pragma unroll
    for (u32 g = 0; g < 8; g++) x[g] = lzp_pick4(in, g * E + p, (g + 8) * E + p, (g + 16) * E + p, (g + 24) * E + p);
    lzb_transpose8(x);
}

// ... and back: w holds, for every byte position p, the eight registers lzb_transpose8 makes of planes 8 p .. 8 p + 7 (byte c of
// w[8 p + g]: byte p of element g + 8 c); registers 4 m .. 4 m + 3 of the interleaved side.
template <u32 E>
LZ_DEV void lzb_from_planes(const u32* w, u32 m, u32* out)
{
#pragma unroll
    for (u32 d = 0; d < 4; d++) {
        u32 s[4];
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            const u32 o = 4 * (4 * m + d) + k, j = o / E, p = o % E;   // the output byte: byte p of element j
            s[k] = (8 * p + j % 8) * 4 + j / 8;
        }
        out[d] = lzp_pick4(w, s[0], s[1], s[2], s[3]);
    }
}

// A 4 x 4 transpose of a[0 .. 3] across the four lanes of a quad: a[c] of lane r <-> a[r] of lane c.  All lanes of the wave call.
// Two stages; in each a lane keeps one register of a pair and takes the other from its partner: a DPP move and a select per
// register and stage.
LZ_DEV void lzb_quad_transpose(u32* a)
{
    const u32 lane = lz_lane();
    const bool odd = (lane & 1u) != 0, high = (lane & 2u) != 0;
#pragma unroll
    for (u32 i = 0; i < 4; i += 2) {
        const u32 t0 = lzb_quad_xor1(a[i]), t1 = lzb_quad_xor1(a[i + 1]);
        a[i] = odd ? t1 : a[i]; a[i + 1] = odd ? a[i + 1] : t0;
    }
#pragma unroll
    for (u32 i = 0; i < 2; i++) {
        const u32 t0 = lzb_quad_xor2(a[i]), t1 = lzb_quad_xor2(a[i + 2]);
        a[i] = high ? t1 : a[i]; a[i + 2] = high ? a[i + 2] : t0;
    }
}

// Elements [e0, e1) of a buffer whose planes have P bytes, e0 a multiple of 2 048 and e1 of 128 (whole quads only): all lanes of
// one wave call and stay together (the quad exchange); e0, e1, P are wave-uniform.  A quad past e1 takes part with zeros and
// touches no memory.  Every register is stored as soon as it is made: the source needs 8 E + 8 registers alive, not twice 8 E
// (the compiler's schedule keeps more: DESIGN.md 8.1 has the counts).
// XOR: xb is the buffer's base (LzPlanesXorEntry), interleaved bytes.  The lane loads from xb the 2 E pieces of 16 bytes that it
// loads from src (split) or is about to store (join: for E >= 2 those are the pieces of the quad it holds after the exchange of
// pieces), together with the source loads of the step, and XORs them in registers: into the source before the transpose, into
// every piece just before its store.
template <u32 E, bool JOIN, bool XOR = false>
LZ_DEV void lzb_move(const u8* src, u8* dst, u64 P, u64 e0, u64 e1, const u8* xb = nullptr)
{
    const u32 lane = lz_lane(), q = lane >> 2, r = lane & 3u;
    constexpr u32 H = E / 2;                                       // groups of four pieces in a lane (the join's exchange of pieces)
    for (u64 base = e0; base < e1; base += LZB_STEP_ELEMS) {
        const bool whole = base + (u64)LZB_QUAD_ELEMS * (q + 1) <= e1;
        const u8* const s = src + (JOIN ? r * P + base / 8 + 16 * q : (base + LZB_LANE_ELEMS * lane) * E);
        u8* const d = dst + (JOIN ? (base + LZB_LANE_ELEMS * lane) * E : r * P + base / 8 + 16 * q);
        u32 in[8 * E];                                             // interleaved: the lane's 32 E bytes; planar: 16 bytes of 2 E planes
        u32 bx[XOR ? 8 * E : 1];                                   // the base's pieces, in the order of the loads (split) or stores (join)
#pragma unroll
        for (u32 m = 0; m < 8 * E; m++) in[m] = 0;
        if (whole) {
#pragma unroll
            for (u32 m = 0; m < 2 * E; m++) lzp_ld16(s + (JOIN ? 4 * m * P : 16 * m), in + 4 * m);
            if constexpr (XOR) {
                // where the lane's piece m lies on the interleaved side: its own 32 E bytes, or (join, E >= 2) piece 4 i + r of the quad's
                const u8* const x = xb + ((JOIN && E >= 2) ? (base + (u64)LZB_QUAD_ELEMS * q) * E + 16 * r : (base + LZB_LANE_ELEMS * lane) * E);
#pragma unroll
                for (u32 m = 0; m < 2 * E; m++) lzp_ld16(x + ((JOIN && E >= 2) ? 64 * m : 16 * m), bx + 4 * m);
                if constexpr (!JOIN) {
#pragma unroll
                    for (u32 m = 0; m < 8 * E; m++) in[m] ^= bx[m];
                }
            }
        }
        if constexpr (!JOIN) {
#pragma unroll
            for (u32 p = 0; p < E; p++) {
                u32 x[8];
                lzb_to_planes<E>(in, p, x);
                lzb_quad_transpose(x);
                lzb_quad_transpose(x + 4);
                if (whole) {
                    lzp_st16(d + (8 * p) * P, x);
                    lzp_st16(d + (8 * p + 4) * P, x + 4);
                }
            }
        } else {
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
                        lzp_st16(d + 16 * m, out);
                    }
                }
            } else {
                // The lane's 32 E bytes are 2 E pieces of 16 bytes.  Stored as they are, a store instruction would put 16 bytes into
                // every 32 E: eight instructions to fill one cache line for E = 4.  So the quad exchanges pieces, four at a time (a
                // 4 x 4 transpose of pieces: four of dwords), and lane r stores piece 4 i + r of the QUAD's 128 E bytes: every
                // store instruction writes runs of 64 contiguous bytes.
                u8* const dq = dst + (base + (u64)LZB_QUAD_ELEMS * q) * E + 16 * r;
#pragma unroll
                for (u32 h = 0; h < H; h++) {
                    u32 o[4][4], t[4][4];                          // o[c][k]: dword k of the lane's piece 4 h + c
#pragma unroll
                    for (u32 c = 0; c < 4; c++) lzb_from_planes<E>(in, 4 * h + c, o[c]);
#pragma unroll
                    for (u32 k = 0; k < 4; k++) {
                        u32 a[4] = { o[0][k], o[1][k], o[2][k], o[3][k] };
                        lzb_quad_transpose(a);                     // a[c]: dword k of piece 4 h + r of lane c
#pragma unroll
                        for (u32 c = 0; c < 4; c++) t[c][k] = a[c];
                    }
                    if (whole) {
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
}

// The ragged end of the planes, elements [n128, n8) (fewer than 128, a multiple of 8), bit by bit: split, a lane per plane byte;
// join, a lane per element byte.  No lane waits for another.
template <u32 E, bool JOIN, bool XOR = false>
LZ_DEV void lzb_ragged(const u8* src, u8* dst, u64 P, u64 n128, u64 n8, const u8* xb = nullptr)
{
    const u32 lane = lz_lane(), R = (u32)(n8 - n128) / 8;          // bytes at the end of every plane: 0 .. 15
    if constexpr (!JOIN) {
        const u32 j = lane & 15u;
        if (j < R)
            for (u32 k = lane >> 4; k < 8 * E; k += 4) {
                u32 v = 0;
                for (u32 b = 0; b < 8; b++) {
                    const u64 at = (n128 + 8 * j + b) * E + k / 8;
                    v |= (((lzp_ld8(src + at) ^ (XOR ? lzp_ld8(xb + at) : 0u)) >> (k % 8)) & 1u) << b;
                }
                lzp_st8(dst + k * P + n128 / 8 + j, v);
            }
    } else {
        for (u32 x = lane; x < 8 * R * E; x += 64) {
            const u64 i = n128 + x / E;
            const u32 p = x % E;
            u32 v = 0;
            for (u32 b = 0; b < 8; b++) v |= ((lzp_ld8(src + (8 * p + b) * P + i / 8) >> (u32)(i % 8)) & 1u) << b;
            lzp_st8(dst + i * E + p, v ^ (XOR ? lzp_ld8(xb + i * E + p) : 0u));
        }
    }
}

template <u32 E, bool JOIN, bool XOR = false>
LZ_DEV void lzb_tile(const u8* src, u8* dst, u64 size, u32 t, const u8* xb = nullptr)
{
    const u64 n = size / E, n8 = n & ~(u64)7, n128 = n & ~(u64)(LZB_QUAD_ELEMS - 1), P = n8 / 8;
    const u64 e0 = (u64)t * (LZP_TILE_BYTES / E);
    const u64 e1 = e0 + LZP_TILE_BYTES / E < n ? e0 + LZP_TILE_BYTES / E : n;
    lzb_move<E, JOIN, XOR>(src, dst, P, e0, e1 < n128 ? e1 : n128, xb);
    if (e1 == n) {                                                 // the buffer's last tile: the ragged end and the copied bytes
        lzb_ragged<E, JOIN, XOR>(src, dst, P, n128, n8, xb);
        const u64 at = n8 * E + lz_lane();                         // fewer than 8 E bytes
        if (at < size) lzp_st8(dst + at, lzp_ld8(src + at) ^ (XOR ? lzp_ld8(xb + at) : 0u));
    }
}

// Tile `tile` (< the batch's tile count) of the batch: all lanes of one wave call; everything but the lane's share is wave-uniform.
template <bool JOIN>
LZ_DEV void lz_bitplanes_tile(const LzPlanesEntry* tab, u32 nEntries, u32 tileOfWave)
{
    const u32 tile = lz_uniform(tileOfWave);                       // in SGPRs: the bisection and the entry are scalar loads
    const LzPlanesEntry* const e = lzp_entry_of(tab, nEntries, tile);
    const u8* const src = (const u8*)(uintptr_t)e->src;
    u8* const dst = (u8*)(uintptr_t)e->dst;
    const u64 size = e->size;
    const u32 E = e->elem, t = tile - e->firstTile;
    if (E == 2) lzb_tile<2, JOIN>(src, dst, size, t);
    else if (E == 4) lzb_tile<4, JOIN>(src, dst, size, t);
    else if (E == 8) lzb_tile<8, JOIN>(src, dst, size, t);
    else lzb_tile<1, JOIN>(src, dst, size, t);
}

// ... of a batch with bases (LzPlanesXorEntry, lzp_xor_entry_of): an entry without a base takes the plain path on a wave-uniform
// branch.
template <bool JOIN, bool XOR>
LZ_DEV void lzb_tile_of(const u8* src, u8* dst, u64 size, u32 E, u32 t, const u8* xb)
{
    if (E == 2) lzb_tile<2, JOIN, XOR>(src, dst, size, t, xb);
    else if (E == 4) lzb_tile<4, JOIN, XOR>(src, dst, size, t, xb);
    else if (E == 8) lzb_tile<8, JOIN, XOR>(src, dst, size, t, xb);
    else lzb_tile<1, JOIN, XOR>(src, dst, size, t, xb);
}

template <bool JOIN>
LZ_DEV void lz_bitplanes_xor_tile(const LzPlanesXorEntry* tab, u32 nEntries, u32 tileOfWave)
{
    const u32 tile = lz_uniform(tileOfWave);
    const LzPlanesXorEntry* const e = lzp_xor_entry_of(tab, nEntries, tile);
    const u8* const src = (const u8*)(uintptr_t)e->src;
    u8* const dst = (u8*)(uintptr_t)e->dst;
    const u8* const xb = (const u8*)(uintptr_t)e->base;
    if (xb) lzb_tile_of<JOIN, true>(src, dst, e->size, e->elem, tile - e->firstTile, xb);
    else lzb_tile_of<JOIN, false>(src, dst, e->size, e->elem, tile - e->firstTile, nullptr);
}

#ifdef __HIPCC__
template <bool JOIN>
LZ_DEV void lz_bitplanes_grid(const LzPlanesEntry* tab, u32 nEntries, u32 nTiles)
{
    const u64 stride = (u64)gridDim.x * LZP_WAVES;
    for (u64 tile = (u64)blockIdx.x * LZP_WAVES + threadIdx.x / 64; tile < nTiles; tile += stride)
        lz_bitplanes_tile<JOIN>(tab, nEntries, (u32)tile);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_bitplanes_split_kernel(const LzPlanesEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_bitplanes_grid<false>(tab, nEntries, nTiles);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_bitplanes_join_kernel(const LzPlanesEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_bitplanes_grid<true>(tab, nEntries, nTiles);
}
template <bool JOIN>
LZ_DEV void lz_bitplanes_xor_grid(const LzPlanesXorEntry* tab, u32 nEntries, u32 nTiles)
{
    const u64 stride = (u64)gridDim.x * LZP_WAVES;
    for (u64 tile = (u64)blockIdx.x * LZP_WAVES + threadIdx.x / 64; tile < nTiles; tile += stride)
        lz_bitplanes_xor_tile<JOIN>(tab, nEntries, (u32)tile);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_bitplanes_xor_split_kernel(const LzPlanesXorEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_bitplanes_xor_grid<false>(tab, nEntries, nTiles);
}
__global__ __launch_bounds__(64 * LZP_WAVES) void lz_bitplanes_xor_join_kernel(const LzPlanesXorEntry* tab, u32 nEntries, u32 nTiles)
{
    lz_bitplanes_xor_grid<true>(tab, nEntries, nTiles);
}
#endif
#endif  /* __cplusplus */
#endif
