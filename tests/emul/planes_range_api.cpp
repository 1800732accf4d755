// tests/emul/planes_range_api.cpp — TEST INFRASTRUCTURE ONLY: the bodies of lizard_amd/csrc/planes_range_kernels.h (lz_planes_range_tile:
// one tile of a batch of element ranges joined out of pieces of their planes) on the CPU SIMT emulator.  Built by
// tests/test_planes_range_emul.py together with simt.cpp into a small library of its own.  lz_ld128 / lz_ld8_s and lz_st128 / lz_st8_s
// — the only names through which the bodies touch a buffer — are redirected to versions that test EVERY access against what the
// tile's item may touch: a read must lie inside one of the item's pieces or its base (the intervals the test hands in), a write
// inside its dst[0 .. (last - first) * E).
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first

unsigned long long lzemu_stats[64];

namespace {
const u64* g_allow;             // pairs (lo, hi) of addresses the current tile may read
u64 g_nAllow, g_wrLo, g_wrHi;
unsigned g_bad;
inline void note_rd(const u8* p, u32 n)
{
    const u64 a = (u64)(uintptr_t)p;
    for (u64 i = 0; i < g_nAllow; i++) if (a >= g_allow[2 * i] && a + n <= g_allow[2 * i + 1]) return;
    g_bad++;
}
inline void note_wr(const u8* p, u32 n) { const u64 a = (u64)(uintptr_t)p; if (a < g_wrLo || a + n > g_wrHi) g_bad++; }
inline lz_u128 traced_ld128(const u8* p) { note_rd(p, 16); return lz_ld128(p); }
inline u8 traced_ld8(const u8* p) { note_rd(p, 1); return lz_ld8_s(p); }
inline void traced_st128(u8* p, lz_u128 v) { note_wr(p, 16); lz_st128(p, v); }
inline void traced_st8(u8* p, u32 v) { note_wr(p, 1); lz_st8_s(p, v); }
}  // namespace
#define lz_ld128 traced_ld128
#define lz_ld8_s traced_ld8
#define lz_st128 traced_st128
#define lz_st8_s traced_st8
#include "../../lizard_amd/csrc/planes_range_kernels.h"
#undef lz_ld128
#undef lz_ld8_s
#undef lz_st128
#undef lz_st8_s

namespace {
struct TileArgs { const LzPlanesRangeEntry* tab; u32 nEntries; const u64* pieces; u32 tile; };
void entry_tile(void* a)
{
    TileArgs* x = (TileArgs*)a;
    lz_planes_range_tile(x->tab, x->nEntries, x->pieces, x->tile);
}
}  // namespace

extern "C" unsigned emul_planes_range_tile_bytes(void) { return LZP_TILE_BYTES; }
extern "C" unsigned emul_planes_range_entry_bytes(void) { return (unsigned)sizeof(LzPlanesRangeEntry); }

// Every tile of the batch, one wave each, tile after tile.  allow[2 * i], allow[2 * i + 1] for i in [allowAt[b], allowAt[b + 1]): the
// address intervals entry b may read.  Returns how many accesses fell outside what their tile's item may touch (the tile's item is
// found here by a plain scan, not by the kernel's bisection).
extern "C" unsigned emul_planes_range(const LzPlanesRangeEntry* tab, unsigned nEntries, const u64* pieces, unsigned nTiles, const u64* allowAt,
                                      const u64* allow, unsigned seed)
{
    unsigned b = 0;
    g_bad = 0;
    for (unsigned tile = 0; tile < nTiles; tile++) {
        TileArgs a = { tab, nEntries, pieces, tile };
        while (b + 1 < nEntries && tab[b + 1].firstTile <= tile) b++;
        g_allow = allow + 2 * allowAt[b]; g_nAllow = allowAt[b + 1] - allowAt[b];
        g_wrLo = tab[b].dst; g_wrHi = tab[b].dst + (tab[b].last - tab[b].first) * tab[b].elem;
        lzemu::run_wave(entry_tile, &a, seed + tile);
    }
    return g_bad;
}
