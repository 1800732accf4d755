// tests/emul/unframe_api.cpp — TEST INFRASTRUCTURE ONLY: the record body of lz_unframe_kernel (lizard_amd/csrc/unframe_kernels.h)
// on the CPU SIMT emulator.  Built by tests/test_unframe_emul.py together with simt.cpp into a small library of its own.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first
#include "../../lizard_amd/csrc/unframe_kernels.h"

unsigned long long lzemu_stats[64];

namespace {
struct RecArgs { const u8* payload; u32 word; u8* slot; u32 cap; u8* stage; u32* ws; u32 result; };
void entry_rec(void* a)
{
    RecArgs* x = (RecArgs*)a;
    const u32 r = lz_unframe_record(x->payload, x->word, x->slot, x->cap, x->stage, x->ws);
    if (lz_lane() == 0) x->result = r;
}
}  // namespace

// One record: `size` payload bytes (the kernel takes the size from the word; the two are passed apart so that a test can see the
// word alone decides), decoded into slot[0..cap).  Returns the decoded size, 0xFFFFFFFE (needs history) or 0xFFFFFFFF.
extern "C" unsigned emul_unframe_record(const void* payload, unsigned size, unsigned word, void* slot, unsigned cap, unsigned seed)
{
    RecArgs a;
    (void)size;
    a.payload = (const u8*)payload; a.word = word; a.slot = (u8*)slot; a.cap = cap; a.result = 0;
    a.stage = (u8*)malloc(4 * LZD_STAGE_BYTES);
    a.ws = (u32*)malloc(4 * LZD_WS_WORDS);
    memset(a.stage, 0xDD, 4 * LZD_STAGE_BYTES);
    memset(a.ws, 0x3C, 4 * LZD_WS_WORDS);
    lzemu::run_wave(entry_rec, &a, seed);
    free(a.stage); free(a.ws);
    return a.result;
}
