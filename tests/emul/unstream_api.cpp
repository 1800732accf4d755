// tests/emul/unstream_api.cpp — TEST INFRASTRUCTURE ONLY: the stream walk of lizard_amd/csrc/unstream_kernels.h (the body of
// lz_unstream_walk_kernel, with lz_unframe_walk of unframe_walk.h inside it) on the CPU SIMT emulator.  Built by
// tests/test_unstream_walk_emul.py together with simt.cpp into a small library of its own.  As in unframe_walk_api.cpp, lz_ld32 /
// lz_ld8_s — the only names through which the bodies read the stream — are redirected to versions that note the lowest and the
// highest address touched, so that a test can assert that nothing outside src[0..srcSize) was read.
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
#include "../../lizard_amd/csrc/unstream_kernels.h"
#undef lz_ld32
#undef lz_ld8_s

namespace {
struct StreamArgs { const u8* src; u64 srcSize; LzStreamCtl* ctl; LzWalkResult* res; u64* offs; u32 tableCap; };
void entry_stream(void* a) { StreamArgs* x = (StreamArgs*)a; lz_unstream_walk(x->src, x->srcSize, x->ctl, x->res, x->offs, x->tableCap); }
}  // namespace

// One launch: from ctl->pos.  readSpan[0..1] = offsets relative to src of the first byte read and of the byte behind the last one
// read (both 0 when nothing was read).
extern "C" void emul_unstream_walk(const void* src, unsigned long long srcSize, LzStreamCtl* ctl, LzWalkResult* res, unsigned long long* offs,
                                   unsigned tableCap, long long* readSpan, unsigned seed)
{
    StreamArgs a = { (const u8*)src, srcSize, ctl, res, (u64*)offs, tableCap };
    g_lo = g_hi = nullptr;
    lzemu::run_wave(entry_stream, &a, seed);
    readSpan[0] = g_lo ? (long long)(g_lo - a.src) : 0;
    readSpan[1] = g_hi ? (long long)(g_hi - a.src) : 0;
}
