// tests/emul/unframes_api.cpp — TEST INFRASTRUCTURE ONLY: the bodies of lizard_amd/csrc/unframes_kernels.h (the batch walk wrapper, the
// settle and the finish of LizardGPU_decompressFrames_device) on the CPU SIMT emulator.  Built by tests/test_unframes_emul.py together
// with simt.cpp into a small library of its own.  As in unframe_walk_api.cpp, lz_ld32 / lz_ld8_s — the only names through which the
// bodies read a frame — are redirected to versions that note the lowest and the highest address touched, here per frame, so that a
// test can assert that nothing outside a frame's src[0..srcSize) was read.
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
#include "../../lizard_amd/csrc/unframes_kernels.h"
#undef lz_ld32
#undef lz_ld8_s

namespace {
struct WalkArgs { const LzUnframesEntry* e; u32 want; u64* offs; u32* words; LzWalkResult* res; };
void entry_walk(void* a) { WalkArgs* x = (WalkArgs*)a; lz_unframes_walk(x->e, x->want, x->offs, x->words, x->res); }

struct SettleArgs { const LzUnframesEntry* e; const u32* out; LzUnframesResult* res; u64* hashBytes; };
void entry_settle(void* a) { SettleArgs* x = (SettleArgs*)a; lz_unframes_settle(x->e, x->out, x->res, x->hashBytes); }

struct FinishArgs { const LzUnframesEntry* frames; u32 nFrames, base; const u32* hashes; LzUnframesResult* results; long long* spans; };
void entry_finish(void* a)                                       // one lane per frame, as in the kernel; the lanes run one after another
{
    FinishArgs* x = (FinishArgs*)a;
    const u32 f = x->base + lz_lane();
    if (f >= x->nFrames) return;
    g_lo = g_hi = nullptr;
    lz_unframes_finish(x->frames + f, x->hashes[f], x->results + f);
    const u8* src = (const u8*)(uintptr_t)x->frames[f].src;
    x->spans[2 * f] = g_lo ? (long long)(g_lo - src) : 0;
    x->spans[2 * f + 1] = g_hi ? (long long)(g_hi - src) : 0;
}
}  // namespace

// One wave per frame, frame after frame.  fill: 0 = count mode (LZU_WALK entries, no tables), 1 = fill mode (LZU_DECODE entries).
// spans[2 f], spans[2 f + 1] = offsets relative to frame f's src of the first byte read and of the byte behind the last one read.
extern "C" void emul_unframes_walk(const LzUnframesEntry* frames, unsigned nFrames, int fill, unsigned long long* offs, unsigned* words,
                                   LzWalkResult* res, long long* spans, unsigned seed)
{
    for (unsigned f = 0; f < nFrames; f++) {
        WalkArgs a = { frames + f, fill ? LZU_DECODE : LZU_WALK, fill ? (u64*)offs : nullptr, fill ? words : nullptr, res + f };
        g_lo = g_hi = nullptr;
        lzemu::run_wave(entry_walk, &a, seed + f);
        const u8* src = (const u8*)(uintptr_t)frames[f].src;
        spans[2 * f] = g_lo ? (long long)(g_lo - src) : 0;
        spans[2 * f + 1] = g_hi ? (long long)(g_hi - src) : 0;
    }
}

extern "C" void emul_unframes_settle(const LzUnframesEntry* frames, unsigned nFrames, const unsigned* out, LzUnframesResult* results,
                                     unsigned long long* hashBytes, unsigned seed)
{
    for (unsigned f = 0; f < nFrames; f++) {
        SettleArgs a = { frames + f, out, results + f, (u64*)hashBytes + f };
        lzemu::run_wave(entry_settle, &a, seed + f);
    }
}

extern "C" void emul_unframes_finish(const LzUnframesEntry* frames, unsigned nFrames, const unsigned* hashes, LzUnframesResult* results,
                                     long long* spans, unsigned seed)
{
    for (unsigned base = 0; base < nFrames; base += 64) {
        FinishArgs a = { frames, nFrames, base, hashes, results, spans };
        lzemu::run_wave(entry_finish, &a, seed + base);
    }
}
