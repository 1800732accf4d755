// tests/emul/count_trip_api.cpp — TEST INFRASTRUCTURE ONLY: the producer / consumer form of levels 10 / 30 (lizard_amd/csrc/lz_split.h)
// on the CPU SIMT emulator with the marks of the count trips and the check bits counted (lz_block.h, LZ_CT_MARK), for batches whose
// blocks lie anywhere in one source area.  Built together with simt.cpp into small libraries of their own by
// tests/test_count_trip_emul.py (one per setting of LZ_BACK_LATE / LZ_CHECK_LO) and into the stand-alone sanitizer
// program tests/count_trip_asan_main.cpp.  Every area a wave is handed is a heap allocation of exactly the size
// lz_fast12_split_kernel declares (lz_kernels.h); as on the device the level-30 producers run without the lane forms, so with the two
// count calls in a row, and the level-10 producers with them.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first
extern "C" unsigned long long lzemu_ct_marks[16];
#define LZ_CT_MARK(i, n) do { if (lz_lane() == 0) __atomic_add_fetch(&lzemu_ct_marks[i], (unsigned long long)(n), __ATOMIC_RELAXED); } while (0)
#include "../../lizard_amd/csrc/lz_block.h"
#include "../../lizard_amd/csrc/lz_split.h"
#include <thread>
#include <vector>

unsigned long long lzemu_stats[64];
unsigned long long lzemu_ct_marks[16];

namespace {
void* exact_area(size_t bytes, int fill)
{
    void* p = nullptr;
    if (posix_memalign(&p, 64, bytes)) abort();
    memset(p, fill, bytes);
    return p;
}
struct SplitWave { LzSplitArgs a; LzSplitShared sh; u32 wave; void* table; u64* ring; u32* hufWs; bool huf; bool lanes; };
void entry_split_init(void* p) { SplitWave* w = (SplitWave*)p; lz_split_shared_init(w->sh, w->a.nProd, w->a.nCons, w->a.nBufs, w->a.qn); }
void entry_split(void* p)
{
    SplitWave* w = (SplitWave*)p;
    if (w->wave < w->a.nProd) { if (w->lanes) lz_split_producer<12, true>(w->a, w->sh, w->wave, w->table, w->ring); else lz_split_producer<12, false>(w->a, w->sh, w->wave, w->table, w->ring); }
    else if (w->huf)          lz_split_consumer<true>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
    else                      lz_split_consumer<false>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
}
}  // namespace

// LZ_BACK_LATE, LZ_CHECK_LO as this library was built
extern "C" void emul_ct_knobs(unsigned out[2]) { out[0] = LZ_BACK_LATE; out[1] = LZ_CHECK_LO; }

// the marks since the last reset (lz_block.h lists them)
extern "C" void emul_ct_marks(unsigned long long out[16], int reset)
{
    for (int i = 0; i < 16; i++) { out[i] = __atomic_load_n(&lzemu_ct_marks[i], __ATOMIC_RELAXED); if (reset) __atomic_store_n(&lzemu_ct_marks[i], 0ull, __ATOMIC_RELAXED); }
}

// Block i is srcSizes[i] bytes at src + srcOffsets[i] -> dst + i * dstStride, sizes[i].  laneForms: < 0 = as the device runs the level
// (level 10 with, level 30 without), else 0 / 1.  Returns 0, -1 = refused.
extern "C" int emul_ct_split(const void* src, int nBlocks, const unsigned long long* srcOffsets, const unsigned* srcSizes, void* dst,
                             int dstStride, unsigned* sizes, int level, int nProd, int nCons, int laneForms, unsigned seed)
{
    const u32 nBufs = 2u + (seed & 1u), qn = (u32)nProd * nBufs <= 32u ? 32u : 64u;
    if ((level != 10 && level != 30) || nProd < 1 || nCons < 1 || nBlocks < 1 || (u32)nProd * nBufs > qn) return -1;
    const bool huf = level >= 30;
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
        x.a = a; x.sh = sh; x.wave = (u32)w; x.huf = huf; x.lanes = laneForms < 0 ? !huf : laneForms != 0;
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
    return 0;
}
