// tests/emul/planes_xor_api.cpp — TEST INFRASTRUCTURE ONLY: the bodies of the XOR-with-base kernels (lz_planes_xor_tile of
// lizard_amd/csrc/planes_kernels.h, lz_bitplanes_xor_tile of bitplanes_kernels.h: one tile of a batch of buffers split into planes
// after an XOR with the buffer's base, or joined and XORed) on the CPU SIMT emulator.  Built by tests/test_planes_xor_emul.py
// together with simt.cpp into a small library of its own.  lz_ld128 / lz_ld8_s and lz_st128 / lz_st8_s — the only names through
// which the bodies touch a buffer — are redirected to versions that judge EVERY access against the tile's buffer: a read lies
// wholly inside src[0..size) or wholly inside base[0..size), a write wholly inside dst[0..size); anything else is counted.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first

unsigned long long lzemu_stats[64];

namespace {
struct Range { const u8* lo; const u8* hi; bool holds(const u8* p, u32 n) const { return lo && p >= lo && p + n <= hi; } };
Range g_src, g_base, g_dst;
unsigned g_bad_rd, g_bad_wr, g_base_rd;
inline void note_rd(const u8* p, u32 n)
{
    if (g_base.holds(p, n)) g_base_rd++;
    else if (!g_src.holds(p, n)) g_bad_rd++;
}
inline void note_wr(const u8* p, u32 n) { if (!g_dst.holds(p, n)) g_bad_wr++; }
inline lz_u128 traced_ld128(const u8* p) { note_rd(p, 16); return lz_ld128(p); }
inline u8 traced_ld8(const u8* p) { note_rd(p, 1); return lz_ld8_s(p); }
inline void traced_st128(u8* p, lz_u128 v) { note_wr(p, 16); lz_st128(p, v); }
inline void traced_st8(u8* p, u32 v) { note_wr(p, 1); lz_st8_s(p, v); }
}  // namespace
#define lz_ld128 traced_ld128
#define lz_ld8_s traced_ld8
#define lz_st128 traced_st128
#define lz_st8_s traced_st8
#include "../../lizard_amd/csrc/bitplanes_kernels.h"     // (includes planes_kernels.h)
#undef lz_ld128
#undef lz_ld8_s
#undef lz_st128
#undef lz_st8_s

namespace {
struct TileArgs { const LzPlanesXorEntry* tab; u32 nEntries, tile; int join, bits; };
void entry_tile(void* a)
{
    TileArgs* x = (TileArgs*)a;
    if (x->bits) {
        if (x->join) lz_bitplanes_xor_tile<true>(x->tab, x->nEntries, x->tile);
        else lz_bitplanes_xor_tile<false>(x->tab, x->nEntries, x->tile);
    } else {
        if (x->join) lz_planes_xor_tile<true>(x->tab, x->nEntries, x->tile);
        else lz_planes_xor_tile<false>(x->tab, x->nEntries, x->tile);
    }
}
}  // namespace

extern "C" unsigned emul_planes_xor_tile_bytes(void) { return LZP_TILE_BYTES; }
extern "C" unsigned emul_planes_xor_entry_bytes(void) { return (unsigned)sizeof(LzPlanesXorEntry); }
extern "C" unsigned emul_planes_entry_bytes(void) { return (unsigned)sizeof(LzPlanesEntry); }

// Every tile of the batch, one wave each, tile after tile.  Returns how many tiles made an access outside their buffer (the tile's
// buffer is found here by a plain scan, not by the kernel's bisection).  *baseReads: the reads that fell inside a base, over the
// whole batch — a test asserts that bases were read at all, and not where there is none.
extern "C" unsigned emul_planes_xor(const LzPlanesXorEntry* tab, unsigned nEntries, unsigned nTiles, int join, int bits, unsigned seed,
                                    unsigned long long* baseReads)
{
    unsigned bad = 0, b = 0;
    unsigned long long reads = 0;
    for (unsigned tile = 0; tile < nTiles; tile++) {
        TileArgs a = { tab, nEntries, tile, join, bits };
        while (b + 1 < nEntries && tab[b + 1].firstTile <= tile) b++;
        const u8* const src = (const u8*)(uintptr_t)tab[b].src;
        const u8* const dst = (const u8*)(uintptr_t)tab[b].dst;
        const u8* const base = (const u8*)(uintptr_t)tab[b].base;
        g_src = Range{ src, src + tab[b].size };
        g_dst = Range{ dst, dst + tab[b].size };
        g_base = base ? Range{ base, base + tab[b].size } : Range{ nullptr, nullptr };
        g_bad_rd = g_bad_wr = g_base_rd = 0;
        lzemu::run_wave(entry_tile, &a, seed + tile);
        if (g_bad_rd || g_bad_wr) bad++;
        reads += g_base_rd;
    }
    if (baseReads) *baseReads = reads;
    return bad;
}
