// tests/pipeline_fake_emul.cpp — TEST INFRASTRUCTURE: the two device bodies the fake launchers of tests/pipeline_fake.c run, on the
// CPU SIMT emulator: the record body of lz_unframe_kernel (tests/emul/unframe_api.cpp, as it is) and the block decoder of
// lz_decompress_kernel (the entry of tests/emul/emul_api.cpp, which cannot be linked beside the former: both define lzemu_stats).
#include "emul/unframe_api.cpp"

namespace {
struct BlockArgs { const u8* in; u32 n; u8* out; u32 cap; u8* stage; u32* ws; u32 result; };
void entry_block_dec(void* a)
{
    BlockArgs* x = (BlockArgs*)a;
    const u32 r = lz_decompress_block(x->in, x->n, x->out, x->cap, x->stage, x->ws);
    if (lz_lane() == 0) x->result = r;
}
}  // namespace

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
