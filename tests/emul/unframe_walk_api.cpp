// tests/emul/unframe_walk_api.cpp — TEST INFRASTRUCTURE ONLY: the frame walk of lizard_amd/csrc/unframe_walk.h on the CPU SIMT
// emulator.  Built by tests/test_unframe_walk_emul.py together with simt.cpp into a small library of its own.
// The walk reads the frame through lz_ld32 / lz_ld8_s alone; here both names are redirected to versions that note the lowest and
// the highest address touched, so that a test can assert that nothing outside src[0..srcSize) was read.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first

unsigned long long lzemu_stats[64];

namespace {
const u8* g_lo; const u8* g_hi;                                  // [g_lo, g_hi): the bytes read so far
inline void note(const u8* p, u32 n) { if (!g_lo || p < g_lo) g_lo = p; if (!g_hi || p + n > g_hi) g_hi = p + n; }
inline u32 traced_ld32(const u8* p) { note(p, 4); return lz_ld32(p); }
inline u8 traced_ld8(const u8* p) { note(p, 1); return lz_ld8_s(p); }
}  // namespace
#define lz_ld32 traced_ld32
#define lz_ld8_s traced_ld8
#include "../../lizard_amd/csrc/unframe_walk.h"
#undef lz_ld32
#undef lz_ld8_s

namespace {
struct WalkArgs { const u8* src; u64 srcSize, startPos, budget, tableCap; u64* offs; u32* words; LzWalkResult* res; };
void entry_walk(void* a)
{
    WalkArgs* x = (WalkArgs*)a;
    lz_unframe_walk(x->src, x->srcSize, x->startPos, x->budget, x->tableCap, x->offs, x->words, x->res);
}
}  // namespace

// One segment.  readSpan[0..1] = offsets relative to src of the first byte read and of the byte behind the last one read
// (both 0 when nothing was read).
extern "C" void emul_unframe_walk(const void* src, unsigned long long srcSize, unsigned long long startPos, unsigned long long budget,
                                  unsigned long long tableCap, unsigned long long* offs, unsigned* words, LzWalkResult* res,
                                  long long* readSpan, unsigned seed)
{
    WalkArgs a;
    a.src = (const u8*)src; a.srcSize = srcSize; a.startPos = startPos; a.budget = budget; a.tableCap = tableCap;
    a.offs = (u64*)offs; a.words = words; a.res = res;
    g_lo = g_hi = nullptr;
    memset(res, 0xEE, sizeof *res);
    lzemu::run_wave(entry_walk, &a, seed);
    readSpan[0] = g_lo ? (long long)(g_lo - a.src) : 0;
    readSpan[1] = g_hi ? (long long)(g_hi - a.src) : 0;
}
