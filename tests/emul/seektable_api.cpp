// tests/emul/seektable_api.cpp — TEST INFRASTRUCTURE ONLY: the body of lz_stream_seektable_kernel (lz_stream_seektable_item of
// lizard_amd/csrc/lz_stream_pack.h: one thread per entry of a seekable stream's table, one more for the frame's header and footer) on
// the CPU SIMT emulator.  Built by tests/test_seek_table_emul.py together with simt.cpp into a small library of its own.  The tables
// are the host file's (lizard_gpu_ctx.h), so the build needs the HIP runtime's headers, as the host C files do.
// The runtime's C++ headers declare a vector type uint4 of their own and the emulator's lz_wave.h a plain struct of that name: the
// runtime's is renamed while its headers are read (nothing here uses it).
#define uint4 lzemu_hip_uint4
#include "../../lizard_amd/csrc/lizard_gpu_ctx.h"
#undef uint4
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — in front of every kernel header

unsigned long long lzemu_stats[64];

#include "../../lizard_amd/csrc/lz_stream_pack.h"

namespace {
struct Args { const LzFramesEntry* frames; const LzStreamEntry* entries; const LzStreamState* state; const u64* offsets; u32 nFrames; u64 fixedTotal, capacity; u32 first; };
void entry_wave(void* a)
{
    const Args* x = (const Args*)a;
    lz_stream_seektable_item(x->frames, x->entries, x->state, x->offsets, x->nFrames, x->fixedTotal, x->capacity, x->first + lz_lane());
}
}  // namespace

extern "C" unsigned emul_seektable_frames_entry_bytes(void) { return (unsigned)sizeof(LzFramesEntry); }
extern "C" unsigned emul_seektable_stream_entry_bytes(void) { return (unsigned)sizeof(LzStreamEntry); }
extern "C" unsigned emul_seektable_state_bytes(void) { return (unsigned)sizeof(LzStreamState); }

// The launch of lz_stream_seektable_launch: nFrames / 256 + 1 workgroups of 256 threads, wave after wave.  Returns the threads run.
extern "C" unsigned emul_seektable(const LzFramesEntry* frames, const LzStreamEntry* entries, const LzStreamState* state, const u64* offsets,
                                   unsigned nFrames, unsigned long long fixedTotal, unsigned long long capacity, unsigned seed)
{
    const u32 threads = (nFrames / 256u + 1u) * 256u;
    for (u32 first = 0; first < threads; first += 64u) {
        Args a = { frames, entries, state, offsets, nFrames, fixedTotal, capacity, first };
        lzemu::run_wave(entry_wave, &a, seed + first);
    }
    return threads;
}
