// tests/emul/sweep_api.cpp — TEST INFRASTRUCTURE ONLY: the two sweeps of the 24-bit LDS table of levels 10 / 30
// (lizard_amd/csrc/lz_block.h: lz_tab_sweep_narrow, one slot per lane and trip, and lz_tab_sweep_wide / lz_tab_fresh_wide, four slots
// per lane and step) on the CPU SIMT emulator, side by side on copies of one table image.  Built by tests/test_wide_sweep_emul.py
// together with simt.cpp into a small library of its own.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first
#include "../../lizard_amd/csrc/lz_block.h"

unsigned long long lzemu_stats[64];

namespace {
struct SweepArgs { void* mem; u32 Ps; int fresh, wide; };
void entry_sweep(void* a)
{
    SweepArgs* x = (SweepArgs*)a;
    const LzTab t = lz_tab_bind<12>(x->mem);
    if (x->wide) { if (x->fresh) lz_tab_fresh_wide<12>(t); else lz_tab_sweep_wide<12>(t, x->Ps); }
    else lz_tab_sweep_narrow<12>(t, x->Ps, x->fresh != 0);
    t.sync();
}
}  // namespace

extern "C" unsigned emul_sweep_table_bytes(void) { return LZ_TAB_BYTES(12); }
// which sweep lz_tab_sweep() — the one the kernels call — is built as in this tree
extern "C" int emul_sweep_default_is_wide(void) { return LZ_WIDE_SWEEP != 0; }

// One wave sweeps the table image at `narrow` with the one-slot sweep and the image at `wide` with the four-slot one, at position Ps
// (fresh: both fill a fresh table, Ps is not used).  Both images are LZ_TAB_BYTES(12) bytes, dword-aligned, and changed in place.
extern "C" void emul_sweep_pair(void* narrow, void* wide, unsigned Ps, int fresh, unsigned seed)
{
    SweepArgs a = { narrow, Ps, fresh, 0 };
    lzemu::run_wave(entry_sweep, &a, seed);
    SweepArgs b = { wide, Ps, fresh, 1 };
    lzemu::run_wave(entry_sweep, &b, seed + 1u);
}
