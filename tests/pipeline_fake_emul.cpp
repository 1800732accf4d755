// tests/pipeline_fake_emul.cpp — TEST INFRASTRUCTURE: the device bodies the fake launchers of tests/pipeline_fake.c run, on the
// CPU SIMT emulator: the record body of lz_unframe_kernel (tests/emul/unframe_api.cpp, as it is), the block decoder of
// lz_decompress_kernel (the entry of tests/emul/emul_api.cpp, which cannot be linked beside the former: both define lzemu_stats)
// and the frame walk of lz_unframe_walk_kernel (as tests/emul/unframe_walk_api.cpp runs it, without its read tracing: here the
// closure that calls it checks the ranges against the fake device's allocations).
#include "emul/unframe_api.cpp"
#include "../lizard_amd/csrc/unframe_walk.h"

namespace {
struct BlockArgs { const u8* in; u32 n; u8* out; u32 cap; u8* stage; u32* ws; u32 result; };
void entry_block_dec(void* a)
{
    BlockArgs* x = (BlockArgs*)a;
    const u32 r = lz_decompress_block(x->in, x->n, x->out, x->cap, x->stage, x->ws);
    if (lz_lane() == 0) x->result = r;
}
struct WalkArgs { const u8* src; u64 srcSize, startPos, budget, tableCap; u64* offs; u32* words; LzWalkResult* res; };
void entry_walk(void* a)
{
    WalkArgs* x = (WalkArgs*)a;
    lz_unframe_walk(x->src, x->srcSize, x->startPos, x->budget, x->tableCap, x->offs, x->words, x->res);
}
}  // namespace

// one segment of lz_unframe_walk_kernel: a single wave
extern "C" void emul_walk_segment(const void* src, unsigned long long srcSize, unsigned long long startPos, unsigned long long budget,
                                  unsigned long long tableCap, unsigned long long* offs, unsigned* words, void* res, unsigned seed)
{
    WalkArgs a;
    a.src = (const u8*)src; a.srcSize = srcSize; a.startPos = startPos; a.budget = budget; a.tableCap = tableCap;
    a.offs = (u64*)offs; a.words = words; a.res = (LzWalkResult*)res;
    lzemu::run_wave(entry_walk, &a, seed);
}

// what lz_decompress_kernel stores in outSizes[b]: the decoded size or LZD_ERR
extern "C" unsigned emul_decompress_block_raw(const void* src, unsigned n, void* dst, unsigned cap, unsigned seed)
{
    BlockArgs a;
    a.in = (const u8*)src; a.n = n; a.out = (u8*)dst; a.cap = cap; a.result = 0;
    a.stage = (u8*)malloc(4 * LZD_STAGE_BYTES);
    a.ws = (u32*)malloc(4 * LZD_WS_WORDS);
    memset(a.stage, 0xDD, 4 * LZD_STAGE_BYTES);
    memset(a.ws, 0x3C, 4 * LZD_WS_WORDS);
    lzemu::run_wave(entry_block_dec, &a, seed);
    free(a.stage); free(a.ws);
    return a.result;
}
