// tests/emul/readahead_api.cpp — TEST INFRASTRUCTURE ONLY: the producer / consumer form of levels 10 / 30 (lizard_amd/csrc/lz_split.h)
// on the CPU SIMT emulator with the source read-ahead's log hook installed (lizard_amd/csrc/lz_touch.h), for batches whose blocks
// lie anywhere in one source area (LzSplitArgs::srcOffsets / ::srcSizes: odd start addresses, a last block that ends at the last
// byte of its allocation).  Built together with simt.cpp into a small library of its own by tests/test_source_readahead_emul.py,
// and into the stand-alone sanitizer program tests/readahead_asan_main.cpp.  Every area a wave is handed is a heap allocation of
// exactly the size lz_fast12_split_kernel declares (lz_kernels.h), as in emul_api.cpp's LZ_EMUL_EXACT_AREAS form; as on the device the
// level-30 producers run without the lane forms, so without the read-ahead.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first
#include "../../lizard_amd/csrc/lz_block.h"
#include "../../lizard_amd/csrc/lz_split.h"
#include <mutex>
#include <thread>
#include <vector>

unsigned long long lzemu_stats[64];

namespace {
void* exact_area(size_t bytes, int fill)
{
    void* p = nullptr;
    if (posix_memalign(&p, 64, bytes)) abort();
    memset(p, fill, bytes);
    return p;
}
// the log: two words per event — the block's source address, then offset | what << 32 (lz_touch_hook_t)
struct Log { std::mutex m; unsigned long long* out; long cap, n; } g_log;
void log_hook(const u8* base, u32 off, int what)
{
    std::lock_guard<std::mutex> lock(g_log.m);
    if (g_log.n < g_log.cap) { g_log.out[2 * g_log.n] = (unsigned long long)(uintptr_t)base; g_log.out[2 * g_log.n + 1] = (unsigned long long)off | ((unsigned long long)what << 32); }
    g_log.n++;
}
struct SplitWave { LzSplitArgs a; LzSplitShared sh; u32 wave; void* table; u64* ring; u32* hufWs; bool huf; };
void entry_split_init(void* p) { SplitWave* w = (SplitWave*)p; lz_split_shared_init(w->sh, w->a.nProd, w->a.nCons, w->a.nBufs, w->a.qn); }
void entry_split(void* p)
{
    SplitWave* w = (SplitWave*)p;
    lz_touch_hook = g_log.out ? log_hook : nullptr;            // (thread-local: every wave is a thread of its own, its lanes run on it)
    if (w->wave < w->a.nProd) { if (w->huf) lz_split_producer<12, false>(w->a, w->sh, w->wave, w->table, w->ring); else lz_split_producer<12, true>(w->a, w->sh, w->wave, w->table, w->ring); }
    else if (w->huf)          lz_split_consumer<true>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
    else                      lz_split_consumer<false>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
}
}  // namespace

// LZ_SRC_READAHEAD, LZ_READAHEAD, LZ_RA_LINE, LZ_RA_PER_ROUND, LZ_RA_AT, LZ_RA_BYTES as this tree builds them
extern "C" void emul_readahead_knobs(unsigned out[6])
{
    out[0] = LZ_SRC_READAHEAD; out[1] = LZ_READAHEAD; out[2] = LZ_RA_LINE; out[3] = LZ_RA_PER_ROUND; out[4] = LZ_RA_AT; out[5] = LZ_RA_BYTES;
}

// Block i is srcSizes[i] bytes at src + srcOffsets[i] -> dst + i * dstStride, sizes[i].  log (may be null): logCap events of two words.
// Returns the number of events the run produced (more than logCap: the log is incomplete), -1 = refused.
extern "C" long emul_readahead_split(const void* src, int nBlocks, const unsigned long long* srcOffsets, const unsigned* srcSizes, void* dst,
                                     int dstStride, unsigned* sizes, int level, int nProd, int nCons, unsigned seed, unsigned long long* log, long logCap)
{
    const u32 nBufs = 2u + (seed & 1u), qn = (u32)nProd * nBufs <= 32u ? 32u : 64u;
    if ((level != 10 && level != 30) || nProd < 1 || nCons < 1 || nBlocks < 1 || (u32)nProd * nBufs > qn) return -1;
    const bool huf = level >= 30;
    g_log.out = log; g_log.cap = logCap; g_log.n = 0;
    LzSplitArgs a;
    a.src = (const u8*)src; a.blockSize = 0; a.nBlocks = (u32)nBlocks; a.lastBlockSize = 0;
    a.srcSizes = srcSizes; a.srcOffsets = (const u64*)srcOffsets; a.activeProd = 0xFFFFFFFFu;
    a.dst = (u8*)dst; a.dstStride = (u64)dstStride; a.sizes = sizes; a.level = (u32)level;
    a.counter = (u32*)exact_area(4, 0);
    a.arena = (u8*)exact_area(LZ_SPLIT_ARENA_BYTES((size_t)nProd, (size_t)nCons, nBufs), 0xC7);
    a.nProd = (u32)nProd; a.nCons = (u32)nCons; a.nBufs = nBufs; a.qn = qn;
    u32* const shared = (u32*)exact_area(4u * LZ_SPLIT_SHARED_WORDS((u32)nProd, (u32)nCons, qn), 0xA5);
    const LzSplitShared sh = lz_split_shared(shared, (u32)nProd, (u32)nCons);
    std::vector<SplitWave> waves((size_t)(nProd + nCons));
    for (int w = 0; w < nProd + nCons; w++) {
        SplitWave& x = waves[(size_t)w];
        x.a = a; x.sh = sh; x.wave = (u32)w; x.huf = huf;
        x.table = w < nProd ? exact_area(4u * (LZ_TAB_BYTES(12) / 4u + 1u), 0x5A) : nullptr;
        x.ring = w < nProd ? (u64*)exact_area(8u * LZ_SEQ_RING, 0xEE) : nullptr;
        x.hufWs = w >= nProd ? (u32*)exact_area(4u * (huf ? LZ_HUF_WS_WORDS : 1u), 0x77) : nullptr;
    }
    lzemu::run_wave(entry_split_init, &waves[0], seed);
    std::vector<std::thread> th;
    for (int w = 0; w < nProd + nCons; w++) th.emplace_back([&waves, w, seed] { lzemu::run_wave(entry_split, &waves[(size_t)w], seed * 31u + (unsigned)w + 1u); });
    for (auto& t : th) t.join();
    for (SplitWave& x : waves) { free(x.table); free(x.ring); free(x.hufWs); }
    free(a.arena); free(shared); free(a.counter);
    g_log.out = nullptr;
    return g_log.n;
}
