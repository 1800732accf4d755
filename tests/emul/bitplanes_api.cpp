// tests/emul/bitplanes_api.cpp — TEST INFRASTRUCTURE ONLY: the bodies of lizard_amd/csrc/bitplanes_kernels.h (lz_bitplanes_tile: one tile
// of a batch of buffers split into bit planes, or joined) on the CPU SIMT emulator.  Built by tests/test_bitplanes_emul.py together
// with simt.cpp into a small library of its own.  lz_ld128 / lz_ld8_s and lz_st128 / lz_st8_s — the only names through which the
// bodies touch a buffer — are redirected to versions that note the lowest and the highest address read and written, per tile, so
// that a test can assert that a tile read nothing outside its buffer's src[0..size) and wrote nothing outside its dst[0..size).
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first

unsigned long long lzemu_stats[64];

namespace {
struct Span { const u8* lo; const u8* hi; void note(const u8* p, u32 n) { if (!lo || p < lo) lo = p; if (!hi || p + n > hi) hi = p + n; } };
Span g_rd, g_wr;
inline lz_u128 traced_ld128(const u8* p) { g_rd.note(p, 16); return lz_ld128(p); }
inline u8 traced_ld8(const u8* p) { g_rd.note(p, 1); return lz_ld8_s(p); }
inline void traced_st128(u8* p, lz_u128 v) { g_wr.note(p, 16); lz_st128(p, v); }
inline void traced_st8(u8* p, u32 v) { g_wr.note(p, 1); lz_st8_s(p, v); }
}  // namespace
#define lz_ld128 traced_ld128
#define lz_ld8_s traced_ld8
#define lz_st128 traced_st128
#define lz_st8_s traced_st8
#include "../../lizard_amd/csrc/bitplanes_kernels.h"
#undef lz_ld128
#undef lz_ld8_s
#undef lz_st128
#undef lz_st8_s

namespace {
struct TileArgs { const LzPlanesEntry* tab; u32 nEntries, tile; int join; };
void entry_tile(void* a)
{
    TileArgs* x = (TileArgs*)a;
    if (x->join) lz_bitplanes_tile<true>(x->tab, x->nEntries, x->tile);
    else lz_bitplanes_tile<false>(x->tab, x->nEntries, x->tile);
}
}  // namespace

extern "C" unsigned emul_bitplanes_tile_bytes(void) { return LZP_TILE_BYTES; }
extern "C" unsigned emul_bitplanes_entry_bytes(void) { return (unsigned)sizeof(LzPlanesEntry); }
extern "C" unsigned emul_bitplanes_step_elems(void) { return LZB_STEP_ELEMS; }

// Every tile of the batch, one wave each, tile after tile.  Returns how many tiles read outside their buffer's src or wrote outside
// its dst (the tile's buffer is found here by a plain scan, not by the kernel's bisection).
extern "C" unsigned emul_bitplanes(const LzPlanesEntry* tab, unsigned nEntries, unsigned nTiles, int join, unsigned seed)
{
    unsigned bad = 0, b = 0;
    for (unsigned tile = 0; tile < nTiles; tile++) {
        TileArgs a = { tab, nEntries, tile, join };
        g_rd = Span{ nullptr, nullptr }; g_wr = Span{ nullptr, nullptr };
        lzemu::run_wave(entry_tile, &a, seed + tile);
        while (b + 1 < nEntries && tab[b + 1].firstTile <= tile) b++;
        const u8* const src = (const u8*)(uintptr_t)tab[b].src;
        const u8* const dst = (const u8*)(uintptr_t)tab[b].dst;
        const bool rd_ok = !g_rd.lo || (g_rd.lo >= src && g_rd.hi <= src + tab[b].size);
        const bool wr_ok = !g_wr.lo || (g_wr.lo >= dst && g_wr.hi <= dst + tab[b].size);
        if (!rd_ok || !wr_ok) bad++;
    }
    return bad;
}
