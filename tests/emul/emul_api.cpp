// tests/emul/emul_api.cpp — TEST INFRASTRUCTURE ONLY: C entry points that run the product's kernel
// bodies (lizard_amd/csrc/lz_block.h, ...) on the CPU SIMT emulator. Loaded by tests via ctypes.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first, see the shared guard
// marks of lz_hc_build's paths (lz_hashchain.h LZ_HC_MARK): counters of their own, read with emul_hc_marks()
extern "C" unsigned long long lzemu_hc_marks[16];
#define LZ_HC_MARK(i) do { if (lz_lane() == 0) __atomic_add_fetch(&lzemu_hc_marks[i], 1ull, __ATOMIC_RELAXED); } while (0)
#include "../../lizard_amd/csrc/lz_block.h"
#include "../../lizard_amd/csrc/lz_unpack.h"
#include "../../lizard_amd/csrc/lz_split.h"
#include <thread>
#include <vector>

namespace {
struct Args { const u8* src; u32 n; u8* dst; u32 level; u32* table; u8* tag; u8* scratch; u64* ring; u32 result; u32 tabKind; u32* hcRegion; u32 maxBlock; u32 poolMask; u32* wideOcc; };

template <int PARSER, int HASHLOG, int AUX, bool HUF>
void entry_block(void* a)
{
    Args* x = (Args*)a;
    LzHufPool hcPool; hcPool.base = x->hcRegion; hcPool.mask = &x->poolMask; hcPool.count = 1; hcPool.stride = LZ_HC_REGION_WORDS;   // a pool of one chain-build region
    u32 r = lz_compress_block<PARSER, HASHLOG, AUX, HUF>(x->src, x->n, x->dst, x->level, x->table, x->tag, x->scratch, x->ring, x->tabKind,
                                                         nullptr, nullptr, 0, &hcPool, x->maxBlock, x->wideOcc, x->wideOcc ? 16u : 0u);
    if (lz_lane() == 0) x->result = r;
}
}  // namespace



unsigned long long lzemu_stats[64];
unsigned long long lzemu_hc_marks[16];
// event counters of the kernels' LZ_STAT marks since the last reset
extern "C" void emul_stats(unsigned long long* out, int reset)
{
    for (int i = 0; i < 64; i++) { out[i] = __atomic_load_n(&lzemu_stats[i], __ATOMIC_RELAXED); if (reset) __atomic_store_n(&lzemu_stats[i], 0ull, __ATOMIC_RELAXED); }
}

// the marks of lz_hc_build since the last reset, `count` (<= 16) of them
extern "C" void emul_hc_marks(unsigned long long* out, int count, int reset)
{
    for (int i = 0; i < count && i < 16; i++) {
        out[i] = __atomic_load_n(&lzemu_hc_marks[i], __ATOMIC_RELAXED);
        if (reset) __atomic_store_n(&lzemu_hc_marks[i], 0ull, __ATOMIC_RELAXED);
    }
}

// What lz_compress_block does in front of the hashChain / noChain parse, and nothing else: lz_hc_begin, lz_hc_build<searchLen, hashLog>
// and lz_hc_hits (pre != 0: levels 16 / 17 / 37 / 38) or lz_hc_hits_plain, on a slot of exactly the size the library gives a wave
// for blocks of n bytes (lizard_gpu.hip ensure_hc_slots: LZ_HC_SLOT_BYTES of n rounded up to 64 KiB, without best[] when pre == 0)
// filled with 0xB7 between 64 canary bytes, and a chain-build region filled with 0x3C3C3C3C.  Copies out prev / chain2 / best for
// p < nIns = n - 7 and the (nIns + 63) / 64 words of hits.  Returns 0, 1 = a canary changed, -1 = no such form.
namespace {
struct HcArgs { const u8* src; u32 n; u32 searchNum; u32 pre; void* slot; u32 maxBlock; u32* region; u32 poolMask; LzHc hc; };
template <int SEARCHLEN, int HLOG>
void entry_hc_tables(void* a)
{
    HcArgs* x = (HcArgs*)a;
    LzHufPool pool; pool.base = x->region; pool.mask = &x->poolMask; pool.count = 1; pool.stride = LZ_HC_REGION_WORDS;
    LzStreams st;
    LzHc hc;
    lz_hc_begin(hc, x->slot, x->maxBlock, x->searchNum);
    lz_hc_build<SEARCHLEN, HLOG>(x->src, x->n, hc, pool, st);
    hc.pre = x->pre != 0u;
    if (x->pre) lz_hc_hits(x->src, x->n, hc); else lz_hc_hits_plain(x->src, x->n, hc);
    if (lz_lane() == 0) x->hc = hc;
}
}  // namespace

extern "C" int emul_hc_tables(const void* src, int n, int searchLen, int hashLog, int searchNum, int pre,
                              unsigned short* prev, unsigned* chain2, unsigned long long* hits, unsigned* best, unsigned seed)
{
    const size_t kGuard = 64;
    const size_t cap = (((size_t)(n > 0 ? n : 1)) + 65535u) & ~(size_t)65535u;
    const size_t slotBytes = LZ_HC_SLOT_BYTES(cap) - (pre ? 0u : 4u * cap);
    void (*fn)(void*) = searchLen == 5 && hashLog == 18 ? entry_hc_tables<5, 18> : searchLen == 4 && hashLog == 18 ? entry_hc_tables<4, 18>
                      : searchLen == 5 && hashLog == 14 ? entry_hc_tables<5, 14> : nullptr;
    if (!fn || n < 0) return -1;
    u8* mem = nullptr;
    if (posix_memalign((void**)&mem, 64, slotBytes + 2 * kGuard)) abort();
    memset(mem, 0xC3, kGuard); memset(mem + kGuard, 0xB7, slotBytes); memset(mem + kGuard + slotBytes, 0xC3, kGuard);
    HcArgs a;
    a.src = (const u8*)src; a.n = (u32)n; a.searchNum = (u32)searchNum; a.pre = (u32)pre; a.slot = mem + kGuard; a.maxBlock = (u32)(n > 0 ? n : 1);
    a.poolMask = 0;
    a.region = (u32*)aligned_alloc(64, (4 * LZ_HC_REGION_WORDS + 63) & ~(size_t)63);
    memset(a.region, 0x3C, 4 * LZ_HC_REGION_WORDS);
    lzemu::run_wave(fn, &a, seed);
    const size_t nIns = n >= 8 ? (size_t)n - 7u : 0u;
    memcpy(prev, a.hc.prev, 2 * nIns);
    memcpy(chain2, a.hc.chain2, 4 * nIns);
    memcpy(hits, a.hc.hits, 8 * ((nIns + 63) / 64));
    if (pre) memcpy(best, a.hc.best, 4 * nIns);
    int bad = a.poolMask != 0u;                                // the region went back
    for (size_t i = 0; i < kGuard; i++) bad |= mem[i] != 0xC3 || mem[kGuard + slotBytes + i] != 0xC3;
    free(mem); free(a.region);
    return bad;
}

#ifndef LZ_EMUL_EXACT_AREAS
// hashChain levels keep one persistent global slot that is never cleared (as the host library does): whatever an earlier
// block left in it (bins, links, saved head tables) must not matter.
static u8* g_hcSlot = nullptr;
static const size_t kHcMaxBlock = 18u << 20;
static u8* hc_slot()
{
    if (!g_hcSlot) { g_hcSlot = (u8*)malloc(LZ_HC_SLOT_BYTES(kHcMaxBlock)); memset(g_hcSlot, 0xB7, LZ_HC_SLOT_BYTES(kHcMaxBlock)); }
    return g_hcSlot;
}

// Compress one block with the emulated wave. dst must hold Lizard_compressBound(n) bytes.
// `seed` drives the lane scheduling order (any value must give identical output).
extern "C" int emul_compress_block(const void* src, int n, void* dst, int level, unsigned seed)
{
    Args a;
    int base = level >= 30 ? level - 20 : level;
    if (level >= 34 && level <= 38) base = level - 21;
    const bool ncLevel = level == 12 || level == 32 || level == 33;       // noChain: the hashChain kernels with one candidate per search
    const bool hcLevel = (base >= 13 && base <= 17) || ncLevel;
    int hashLog = ncLevel ? (level == 32 ? 14 : 18) : base == 10 ? 12 : base == 11 ? 18 : base == 20 ? 14 : base == 21 ? 14 : base == 22 ? 18 : hcLevel ? 18 : 0;
    if (!hashLog) return -1;
    if (hcLevel && (size_t)n > kHcMaxBlock) return -1;
    a.src = (const u8*)src; a.n = (u32)n; a.dst = (u8*)dst; a.level = (u32)level; a.result = 0;
    // odd seeds run the u32-slot (global-memory) table layout of the mixed-residency kernels; seeds = 2 mod 4 the packed
    // 18 + 6 bit LDS table of the priceFast kernel for blocks up to 256 KiB; the others the u32-slot LDS form
    a.tabKind = (base == 20 || ((base == 21 || base == 22 || base == 10) && (seed & 1u))) ? LZ_TABKIND_GLOBAL
              : (base == 21 && n <= (1 << 18) && (seed & 3u) == 2u) ? LZ_TABKIND_LDS18 : LZ_TABKIND_LDS;
    a.table = (u32*)aligned_alloc(64, (sizeof(u32) << hashLog) + 64);
    a.tag = (u8*)malloc(8192);
    a.scratch = (u8*)malloc(LZ_SCRATCH_BYTES);
    u64 ring[LZ_SEQ_RING]; memset(ring, 0xEE, sizeof ring); a.ring = ring;
    memset(a.table, 0xA5, (sizeof(u32) << hashLog) + 64);   // garbage: the kernel must initialise its state
    memset(a.tag, 0x5A, 8192);
    memset(a.scratch, 0xCC, LZ_SCRATCH_BYTES);
    static_assert(4 * LZ_HUF_WS_WORDS <= 8192, "emulated LDS workspace too small");
    const bool huf = level >= 30;
    void* garbageTable = a.table;
    if (hcLevel) a.table = (u32*)hc_slot();
    a.maxBlock = (u32)kHcMaxBlock; a.poolMask = 0;
    a.wideOcc = ((base == 11 || base == 22 || base == 20) && !(seed & 2u)) ? (u32*)malloc(8192 + 8) : nullptr;     // levels 11/31, 22/42: with and without the occupancy summary; 20/40: with and without the slot codes
    if (a.wideOcc) memset(a.wideOcc, 0x77, 8192 + 8);
    a.hcRegion = (u32*)aligned_alloc(64, 4 * LZ_HC_REGION_WORDS + 64);
    memset(a.hcRegion, 0x3C, 4 * LZ_HC_REGION_WORDS);
    if (level == 32) lzemu::run_wave(entry_block<LZ_PARSER_HASHCHAIN, 14, 6, true>, &a, seed);
    else if (ncLevel) lzemu::run_wave(huf ? entry_block<LZ_PARSER_HASHCHAIN, 18, 6, true> : entry_block<LZ_PARSER_HASHCHAIN, 18, 6, false>, &a, seed);
    else switch (base) {
    case 13:                   lzemu::run_wave(huf ? entry_block<LZ_PARSER_HASHCHAIN, 18, 7, true> : entry_block<LZ_PARSER_HASHCHAIN, 18, 7, false>, &a, seed); break;
    case 14:                   lzemu::run_wave(huf ? entry_block<LZ_PARSER_HASHCHAIN, 18, 8, true> : entry_block<LZ_PARSER_HASHCHAIN, 18, 8, false>, &a, seed); break;
    case 15:                   lzemu::run_wave(huf ? entry_block<LZ_PARSER_HASHCHAIN, 18, 9, true> : entry_block<LZ_PARSER_HASHCHAIN, 18, 9, false>, &a, seed); break;
    case 16: case 17:          lzemu::run_wave(huf ? entry_block<LZ_PARSER_HASHCHAIN, 18, 4, true> : entry_block<LZ_PARSER_HASHCHAIN, 18, 4, false>, &a, seed); break;
    case 10: lzemu::run_wave(huf ? entry_block<LZ_PARSER_FAST, 12, 0, true> : entry_block<LZ_PARSER_FAST, 12, 0, false>, &a, seed); break;
    case 11: lzemu::run_wave(huf ? entry_block<LZ_PARSER_FAST, 18, 0, true> : entry_block<LZ_PARSER_FAST, 18, 0, false>, &a, seed); break;
    case 20: lzemu::run_wave(huf ? entry_block<LZ_PARSER_FASTBIG, 14, 10, true> : entry_block<LZ_PARSER_FASTBIG, 14, 10, false>, &a, seed); break;
    case 21: lzemu::run_wave(huf ? entry_block<LZ_PARSER_PRICEFAST, 14, 12, true> : entry_block<LZ_PARSER_PRICEFAST, 14, 12, false>, &a, seed); break;
    default: lzemu::run_wave(huf ? entry_block<LZ_PARSER_PRICEFAST, 18, 12, true> : entry_block<LZ_PARSER_PRICEFAST, 18, 12, false>, &a, seed); break;
    }
    free(garbageTable); free(a.tag); free(a.scratch); free(a.hcRegion); free(a.wideOcc);
    return (int)a.result;
}

#else   /* LZ_EMUL_EXACT_AREAS */
// -DLZ_EMUL_EXACT_AREAS (tests/emul_asan_main.cpp under AddressSanitizer): every area a kernel body is handed is a heap allocation
// of its own with exactly the size the product gives it, so that the sanitizer's redzones sit where the neighbouring wave's
// slice, the next table slot or the next scratch slot begins on the device.  The template arguments, the table kind and the
// pool / summary / tag sizes are those of the kernel that serves the level (lz_kernels.h), not the roomier ones of the default
// build above; each size below names the declaration it restates.
namespace {
void* exact_area(size_t bytes, int fill)
{
    void* p = nullptr;
    if (posix_memalign(&p, 64, bytes)) abort();              // the start is aligned, the END is exact: nothing is rounded
    memset(p, fill, bytes);                                  // garbage: the kernel must initialise its state
    return p;
}
struct XArgs { const u8* src; u32 n; u8* dst; u32 level; void* table; u8* ws; u8* scratch; u64* ring; u32 result; u32 tabKind;
               u32* hufPool; u32 hufPoolMask; u32 hufPoolCount; u32* hcRegion; u32 hcPoolMask; u32 maxBlock; u32* occ; u32 occLog; u32 tagLog; };
template <int PARSER, int HASHLOG, int AUX, bool HUF>
void entry_exact(void* a)
{
    XArgs* x = (XArgs*)a;
    LzHufPool hcPool; hcPool.base = x->hcRegion; hcPool.mask = &x->hcPoolMask; hcPool.count = 1; hcPool.stride = LZ_HC_REGION_WORDS;   // a pool of one region
    u32 r = lz_compress_block<PARSER, HASHLOG, AUX, HUF>(x->src, x->n, x->dst, x->level, x->table, x->ws, x->scratch, x->ring, x->tabKind,
                                                         x->hufPoolCount ? x->hufPool : nullptr, x->hufPoolCount ? &x->hufPoolMask : nullptr, x->hufPoolCount,
                                                         &hcPool, x->maxBlock, x->occ, x->occLog, x->tagLog);
    if (lz_lane() == 0) x->result = r;
}
template <int PARSER, int HASHLOG, int AUX>
void run_exact(bool huf, XArgs* a, unsigned seed) { lzemu::run_wave(huf ? entry_exact<PARSER, HASHLOG, AUX, true> : entry_exact<PARSER, HASHLOG, AUX, false>, a, seed); }
}  // namespace

// Same contract as the default build's entry.  Which form of a level runs follows the seed as it does there, but only forms that a
// kernel of lizard_amd/csrc declares are run (levels 22 / 42 have no LDS-table form, level 10 no global-table form).
extern "C" int emul_compress_block(const void* src, int n, void* dst, int level, unsigned seed)
{
    const bool huf = level >= 30;
    int base = huf ? level - 20 : level;
    if (level >= 34 && level <= 38) base = level - 21;
    const bool ncLevel = level == 12 || level == 32 || level == 33;
    const bool hcLevel = (base >= 13 && base <= 17) || ncLevel;
    if (!hcLevel && base != 10 && base != 11 && base != 20 && base != 21 && base != 22) return -1;
    if (n < 1) return -1;
    XArgs a; memset(&a, 0, sizeof a);
    a.src = (const u8*)src; a.n = (u32)n; a.dst = (u8*)dst; a.level = (u32)level; a.tagLog = LZ_WIDE_TAGLOG;
    a.tabKind = LZ_TABKIND_LDS;
    // per wave, every kernel: Slice::ring[LZ_SEQ_RING] (lz_kernels.h:79) and one scratch slot of LZ_SCRATCH_BYTES (lz_kernels.h:105)
    a.ring = (u64*)exact_area(8u * LZ_SEQ_RING, 0xEE);
    a.scratch = (u8*)exact_area(LZ_SCRATCH_BYTES, 0xCC);
    size_t tableBytes = 0, wsWords = 1;                          // Slice::ws[WSWORDS] (lz_kernels.h:79); WSWORDS = 1 where the wave has no use for it
    u32 pool = 0;                                                // Huffman workspaces from hufPool[POOL][LZ_HUF_WS_WORDS] (lz_kernels.h:89): one of them here
    bool occ = false;                                            // wideOcc[..][kOccWords], kOccWords = (2^OCCLOG >> 5) + 1 (lz_kernels.h:94-95)
    const size_t kWsOwn = LZ_HUF_WS_WORDS, kTags1K = (1u << 10) / 4u;
    const size_t kPfSlotBytes = 65536u;                          // LZ_PF_SLOT_BYTES (lz_kernels.h:276; that file is device-only)
    int pfAux = 11;                                              // level 21 / 41: the AUX (TAGLOG) of the form that runs
    if (hcLevel) {
        // lz_hashchain_kernel (lz_kernels.h:218): WSWORDS = LZ_HUF_WS_WORDS with the Huffman stage (LZ_HC_HUF_POOL 0), else 1; the table is
        // the wave's work area: LZ_HC_SLOT_BYTES of the block size rounded up to 64 KiB, without best[] below levels 16 / 37
        // (lizard_gpu.hip:405-409, :316 needBest), laid out for maxBlock = the launch's block size (lz_kernels.h:128); the chain build
        // borrows hcPoolMem[..][LZ_HC_REGION_WORDS] (lz_kernels.h:97)
        const size_t cap = ((size_t)n + 65535u) & ~(size_t)65535u;
        const bool needBest = base >= 16 && !ncLevel;
        tableBytes = LZ_HC_SLOT_BYTES(cap) - (needBest ? 0u : 4u * cap);
        wsWords = huf ? kWsOwn : 1;
        a.maxBlock = (u32)n;
        a.hcRegion = (u32*)exact_area(4u * LZ_HC_REGION_WORDS, 0x3C);
    } else if (base == 10) {
        // variants/lz_fast12_onewave.h:14-18 (the library itself runs levels 10 / 30 in the split form below).  Level 10: every table
        // in LDS, WSWORDS 1.  Level 30, by seed: a global-table wave of the mixed form (a 64 KiB slot, lizard_gpu.hip:129 kPf64k; tags
        // wideTags[..][2^LZ_WIDE_TAGLOG / 4], lz_kernels.h:100-101; pooled workspace), an LDS-table wave of it (WSWORDS 1, pooled
        // workspace), or the all-LDS form (WSWORDS = LZ_HUF_WS_WORDS).  LDS table: kTabWords = LZ_TAB_BYTES(12) / 4 + 1 (lz_kernels.h:80)
        tableBytes = 4u * (LZ_TAB_BYTES(12) / 4u + 1u);
        if (huf && (seed & 1u)) { a.tabKind = LZ_TABKIND_GLOBAL; tableBytes = kPfSlotBytes; wsWords = (1u << LZ_WIDE_TAGLOG) / 4u; pool = 1; }
        else if (huf && (seed & 3u) == 0u) pool = 1;
        else if (huf) wsWords = kWsOwn;
    } else if (base == 11) {
        // lz_fast18_kernel (lz_kernels.h:199-200): WSWORDS = 2^10 / 4 (the 1 KiB tag array, WIDETAGLOG 10), OCCLOG 16, level 31 a pooled
        // workspace (LZ_WIDE_HUF_POOL 4); the table slot is LZ_TABWIDE_BYTES(18) (lizard_gpu.hip:129 kWide18)
        a.tabKind = LZ_TABKIND_GLOBAL; tableBytes = LZ_TABWIDE_BYTES(18); wsWords = kTags1K; a.tagLog = 10; pool = huf; occ = !(seed & 2u);
    } else if (base == 20) {
        // lz_fastbig14_kernel (lz_kernels.h:235-236): WSWORDS = 2^10 / 4, OCCLOG 16 (the slot codes), level 40 a pooled workspace; the
        // table is a 64 KiB slot (lizard_gpu.hip:129 kPf64k, LZ_PF_SLOT_BYTES lz_kernels.h:276)
        a.tabKind = LZ_TABKIND_GLOBAL; tableBytes = kPfSlotBytes; wsWords = kTags1K; pool = huf; occ = !(seed & 2u);
    } else if (base == 21) {
        // lz_pricefast14_kernel (lz_kernels.h:283-288).  SMALL (blocks <= 256 KiB): AUX 10, WSWORDS 1, level 41 a pooled workspace; LDS
        // tables kTabWords = LZ_TAB24C_BYTES(14) / 4 + 1; the global-table waves' tags wideTags[..][2^AUX / 4] (lz_kernels.h:100-101).
        // General: AUX 11, WSWORDS = LZ_HUF_WS_WORDS at level 41 (it doubles as the tag array) else 1 and wideTags of 2^11 / 4 words;
        // LDS tables kTabWords = (4 << 14) / 4 + 1.  Global tables: a 64 KiB slot.
        const bool small = n <= (1 << 18) && (seed & 3u) != 0u;                   // seed 0 mod 4: the general form at every size
        if (seed & 1u) { a.tabKind = LZ_TABKIND_GLOBAL; tableBytes = kPfSlotBytes; }
        else if (small) { a.tabKind = LZ_TABKIND_LDS18; tableBytes = 4u * (LZ_TAB24C_BYTES(14) / 4u + 1u); }
        else tableBytes = 4u * ((4u << 14) / 4u + 1u);
        if (small) { wsWords = (seed & 1u) ? kTags1K : 1; pool = huf; }
        else wsWords = huf ? kWsOwn : (seed & 1u) ? (1u << 11) / 4u : 1;
        pfAux = small ? 10 : 11;
    } else {
        // lz_pricefast18_kernel (lz_kernels.h:297-298): AUX 10, WSWORDS = 2^10 / 4, OCCLOG 16, level 42 a pooled workspace; every table is
        // a global slot of LZ_TABWIDE_BYTES(18) (lizard_gpu.hip:129 kWide18)
        a.tabKind = LZ_TABKIND_GLOBAL; tableBytes = LZ_TABWIDE_BYTES(18); wsWords = kTags1K; pool = huf; occ = !(seed & 2u);
    }
    a.table = exact_area(tableBytes, hcLevel ? 0xB7 : 0xA5);
    a.ws = (u8*)exact_area(4u * wsWords, 0x5A);
    if (pool) { a.hufPool = (u32*)exact_area(4u * LZ_HUF_WS_WORDS, 0x77); a.hufPoolCount = 1; }
    if (occ) { a.occLog = 16; a.occ = (u32*)exact_area(4u * (((1u << 16) >> 5) + 1u), 0x77); }
    if (level == 32) run_exact<LZ_PARSER_HASHCHAIN, 14, 6>(true, &a, seed);
    else if (ncLevel) run_exact<LZ_PARSER_HASHCHAIN, 18, 6>(huf, &a, seed);
    else switch (base) {
    case 13: run_exact<LZ_PARSER_HASHCHAIN, 18, 7>(huf, &a, seed); break;
    case 14: run_exact<LZ_PARSER_HASHCHAIN, 18, 8>(huf, &a, seed); break;
    case 15: run_exact<LZ_PARSER_HASHCHAIN, 18, 9>(huf, &a, seed); break;
    case 16: case 17: run_exact<LZ_PARSER_HASHCHAIN, 18, 4>(huf, &a, seed); break;
    case 10: run_exact<LZ_PARSER_FAST, 12, 0>(huf, &a, seed); break;
    case 11: run_exact<LZ_PARSER_FAST, 18, 0>(huf, &a, seed); break;
    case 20: run_exact<LZ_PARSER_FASTBIG, 14, 10>(huf, &a, seed); break;
    case 21: if (pfAux == 10) run_exact<LZ_PARSER_PRICEFAST, 14, 10>(huf, &a, seed); else run_exact<LZ_PARSER_PRICEFAST, 14, 11>(huf, &a, seed); break;
    default: run_exact<LZ_PARSER_PRICEFAST, 18, 10>(huf, &a, seed); break;
    }
    free(a.ring); free(a.scratch); free(a.table); free(a.ws); free(a.hufPool); free(a.occ); free(a.hcRegion);
    return (int)a.result;
}
#endif  /* LZ_EMUL_EXACT_AREAS */

// One Huffman-candidate stream through lz_put_stream_huf (Lizard_writeStream semantics):
// out receives LE24 n ‖ LE24 c ‖ payload (accepted) or LE24 n ‖ raw bytes; returns bytes written,
// *huffed tells which.
namespace {
struct HufArgs { const u8* stream; u32 n; u8* out; u32* ws; u32 result; u32 huffed; };
void entry_huf(void* a)
{
    HufArgs* x = (HufArgs*)a;
    u32 h = 0;
    u32 r = lz_put_stream_huf(x->out, x->stream, x->n, x->ws, &h);
    if (lz_lane() == 0) { x->result = r; x->huffed = h; }
}
}  // namespace

extern "C" int emul_put_stream_huf(const void* stream, int n, void* out, int* huffed, unsigned seed)
{
    HufArgs a;
    a.stream = (const u8*)stream; a.n = (u32)n; a.out = (u8*)out; a.result = 0; a.huffed = 0;
    a.ws = (u32*)malloc(4 * LZ_HUF_WS_WORDS);
    memset(a.ws, 0x77, 4 * LZ_HUF_WS_WORDS);
    lzemu::run_wave(entry_huf, &a, seed);
    free(a.ws);
    *huffed = (int)a.huffed;
    return (int)a.result;
}

// `count` streams one after the other through ONE workspace that is filled with 0x77 before the first and never touched between
// them — the product runs the flag stream and the literal stream of a sub-block through the same workspace (lz_write_subblock_seq).
// Stream i: ns[i] bytes at src + srcAt[i] -> out + outAt[i]; sizes[i] / huffed[i] receive what the stage returned.
extern "C" void emul_put_streams_huf(const void* src, const unsigned long long* srcAt, const int* ns, int count, void* out,
                                     const unsigned long long* outAt, int* sizes, int* huffed, unsigned seed)
{
    u32* const ws = (u32*)malloc(4 * LZ_HUF_WS_WORDS);
    memset(ws, 0x77, 4 * LZ_HUF_WS_WORDS);
    for (int i = 0; i < count; i++) {
        HufArgs a;
        a.stream = (const u8*)src + srcAt[i]; a.n = (u32)ns[i]; a.out = (u8*)out + outAt[i]; a.ws = ws; a.result = 0; a.huffed = 0;
        lzemu::run_wave(entry_huf, &a, seed + (unsigned)i);
        sizes[i] = (int)a.result; huffed[i] = (int)a.huffed;
    }
    free(ws);
}


// Wave-wide helpers of lz_block.h against scalar definitions on one buffer: forward/backward common lengths
// (lz_count_fwd, lz_count_back, lz_count_both), lz_copy and the scan/reduce primitives.  Returns the number of
// disagreements (0 = all good).  `pairs` = n triples (P, M, limitOrAnchor) with M < P.
namespace {
struct HelperArgs { const u8* buf; u32 n; const u32* trip; u32 ntrip; u8* tmp; u32 bad; };
void entry_helpers(void* a)
{
    HelperArgs* x = (HelperArgs*)a;
    const u32 lane = lz_lane();
    u32 bad = 0;
    for (u32 t = 0; t < x->ntrip; t++) {
        const u32 P = x->trip[3 * t], M = x->trip[3 * t + 1], lim = x->trip[3 * t + 2];   // M < P <= lim <= n - 16
        // scalar definitions
        u32 f = 0; while (P + f < lim && x->buf[P + f] == x->buf[M + f]) f++;
        const u32 anchor = M > P / 2u ? P / 2u : M / 2u;                                       // some anchor <= P
        u32 b = 0; while (P - b > anchor && M - b > 0u && x->buf[P - b - 1u] == x->buf[M - b - 1u]) b++;
        const u32 gf = lz_count_fwd(x->buf, P, M, lim);
        const u32 gb = lz_count_back(x->buf, P, M, anchor);
        u32 hf = 0, hb = 0;
        lz_count_both(x->buf, P, M, lim, anchor, hf, hb);
        if (gf != f || gb != b || hf != f || hb != b) bad++;
        // copy of the matched span into tmp and back-check
        const u32 len = f < 3000u ? f + (t & 7u) : 3000u;
        lz_copy(x->tmp, x->buf + M, len);
        lz_wave_sync();
        u32 diff = 0;
        for (u32 i = lane; i < len; i += 64u) diff += x->tmp[i] != x->buf[M + i];
        if (lz_wave_reduce_add(diff)) bad++;
        lz_wave_sync();
        // scans: values derived from the data
        const u32 v = x->buf[(P + lane) % x->n];
        const u32 ex = lz_wave_scan_excl_add(v);
        u32 want = 0; for (u32 l = 0; l < lane; l++) want += x->buf[(P + l) % x->n];
        u32 mx = 0; for (u32 l = 0; l < 64u; l++) { const u32 w = x->buf[(P + l) % x->n]; mx = w > mx ? w : mx; }
        const u64 wrong = lz_ballot(ex != want);
        if (wrong || lz_readlane(lz_wave_reduce_max(v), 63u) != mx) bad++;
    }
    if (lane == 0) x->bad = bad;
}
}  // namespace

extern "C" int emul_check_helpers(const void* buf, int n, const unsigned* triples, int ntriples, unsigned seed)
{
    HelperArgs a;
    a.buf = (const u8*)buf; a.n = (u32)n; a.trip = triples; a.ntrip = (u32)ntriples; a.bad = 0;
    a.tmp = (u8*)malloc(4096);
    lzemu::run_wave(entry_helpers, &a, seed);
    free(a.tmp);
    return (int)a.bad;
}


// One block through the product's decoder body (lz_unpack.h).  Returns the decoded size, -1 = refused.
namespace {
struct DecArgs { const u8* in; u32 n; u8* out; u32 cap; u8* stage; u32* ws; u32 result; };
void entry_dec(void* a)
{
    DecArgs* x = (DecArgs*)a;
    const u32 r = lz_decompress_block(x->in, x->n, x->out, x->cap, x->stage, x->ws);
    if (lz_lane() == 0) x->result = r;
}
}  // namespace

extern "C" int emul_decompress_block(const void* src, int n, void* dst, int cap, unsigned seed)
{
    DecArgs a;
    a.in = (const u8*)src; a.n = (u32)n; a.out = (u8*)dst; a.cap = (u32)cap; a.result = 0;
    a.stage = (u8*)malloc(4 * LZD_STAGE_BYTES);
    a.ws = (u32*)malloc(4 * LZD_WS_WORDS);
    memset(a.stage, 0xDD, 4 * LZD_STAGE_BYTES);
    memset(a.ws, 0x3C, 4 * LZD_WS_WORDS);
    lzemu::run_wave(entry_dec, &a, seed);
    free(a.stage); free(a.ws);
    return a.result == LZD_ERR ? -1 : (int)a.result;
}


// Levels 10 / 30 in the producer / consumer form (lizard_amd/csrc/lz_split.h): nProd + nCons emulated waves, each on an OS thread
// of its own, share one "LDS" (mailboxes, free masks, counters) and one scratch arena, exactly as the waves of one workgroup of
// lz_fast12_split_kernel do.  Block i is src + i*blockSize (the last one lastBlockSize bytes) -> dst + i*dstStride, sizes[i].
namespace {
struct SplitWave { LzSplitArgs a; LzSplitShared sh; u32 wave; void* table; u64* ring; u32* hufWs; bool huf; };
void entry_split_init(void* p) { SplitWave* w = (SplitWave*)p; lz_split_shared_init(w->sh, w->a.nProd, w->a.nCons, w->a.nBufs, w->a.qn); }
void entry_split(void* p)
{
    SplitWave* w = (SplitWave*)p;
    if (w->wave < w->a.nProd) lz_split_producer<12>(w->a, w->sh, w->wave, w->table, w->ring);
    else if (w->huf)          lz_split_consumer<true>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
    else                      lz_split_consumer<false>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
}
#ifdef LZ_EMUL_EXACT_AREAS
void entry_split_exact(void* p)
{
    SplitWave* w = (SplitWave*)p;
    if (w->wave < w->a.nProd) { if (w->huf) lz_split_producer<12, false>(w->a, w->sh, w->wave, w->table, w->ring); else lz_split_producer<12, true>(w->a, w->sh, w->wave, w->table, w->ring); }
    else if (w->huf)          lz_split_consumer<true>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
    else                      lz_split_consumer<false>(w->a, w->sh, w->wave - w->a.nProd, w->hufWs);
}
#endif
}  // namespace

// srcSizes / activeProd: the ragged batches and the producer cap of small launches (LzBatch::srcSizes, ::activeWaves); nullptr / 0 = off
extern "C" int emul_compress_split_ragged(const void* src, int nBlocks, int blockSize, int lastBlockSize, const unsigned* srcSizes, void* dst,
                                          int dstStride, unsigned* sizes, int level, int nProd, int nCons, int activeProd, unsigned seed);
extern "C" int emul_compress_split(const void* src, int nBlocks, int blockSize, int lastBlockSize, void* dst, int dstStride,
                                   unsigned* sizes, int level, int nProd, int nCons, unsigned seed)
{
    return emul_compress_split_ragged(src, nBlocks, blockSize, lastBlockSize, nullptr, dst, dstStride, sizes, level, nProd, nCons, 0, seed);
}
#ifndef LZ_EMUL_EXACT_AREAS
extern "C" int emul_compress_split_ragged(const void* src, int nBlocks, int blockSize, int lastBlockSize, const unsigned* srcSizes, void* dst,
                                          int dstStride, unsigned* sizes, int level, int nProd, int nCons, int activeProd, unsigned seed)
{
    const u32 nBufs = 2u + (seed & 1u), qn = 64u;              // odd seeds: three buffers per producer
    if ((level != 10 && level != 30) || nProd < 1 || nCons < 1 || (u32)nProd * nBufs > qn) return -1;
    LzSplitArgs a;
    a.src = (const u8*)src; a.blockSize = (u64)blockSize; a.nBlocks = (u32)nBlocks; a.lastBlockSize = (u32)lastBlockSize;
    a.srcSizes = srcSizes; a.activeProd = activeProd > 0 ? (u32)activeProd : 0xFFFFFFFFu;
    a.dst = (u8*)dst; a.dstStride = (u64)dstStride; a.sizes = sizes; a.level = (u32)level;
    u32 counter = 0; a.counter = &counter;
    const size_t arenaBytes = LZ_SPLIT_ARENA_BYTES((size_t)nProd, (size_t)nCons, nBufs);
    a.arena = (u8*)malloc(arenaBytes); memset(a.arena, 0xC7, arenaBytes);
    a.nProd = (u32)nProd; a.nCons = (u32)nCons; a.nBufs = nBufs; a.qn = qn;
    std::vector<u32> shared(LZ_SPLIT_SHARED_WORDS((u32)nProd, (u32)nCons, qn), 0xA5A5A5A5u);
    const LzSplitShared sh = lz_split_shared(shared.data(), (u32)nProd, (u32)nCons);
    const size_t tabBytes = LZ_TAB_BYTES(12) + 64;
    std::vector<u8> tables((size_t)nProd * tabBytes, 0x5A);
    std::vector<u64> rings((size_t)nProd * LZ_SEQ_RING, 0xEEEEEEEEEEEEEEEEull);
    std::vector<u32> ws((size_t)nCons * LZ_HUF_WS_WORDS, 0x77777777u);
    std::vector<SplitWave> waves((size_t)(nProd + nCons));
    for (int w = 0; w < nProd + nCons; w++) {
        SplitWave& x = waves[(size_t)w];
        x.a = a; x.sh = sh; x.wave = (u32)w; x.huf = level >= 30;
        x.table = w < nProd ? (void*)&tables[(size_t)w * tabBytes] : nullptr;
        x.ring = w < nProd ? &rings[(size_t)w * LZ_SEQ_RING] : nullptr;
        x.hufWs = w >= nProd ? &ws[(size_t)(w - nProd) * LZ_HUF_WS_WORDS] : nullptr;
    }
    lzemu::run_wave(entry_split_init, &waves[0], seed);
    std::vector<std::thread> th;
    for (int w = 0; w < nProd + nCons; w++) th.emplace_back([&waves, w, seed] { lzemu::run_wave(entry_split, &waves[(size_t)w], seed * 31u + (unsigned)w + 1u); });
    for (auto& t : th) t.join();
    free(a.arena);
    return 0;
}
#else   /* LZ_EMUL_EXACT_AREAS */
// The split form with every area exact and on the heap: what lz_fast12_split_kernel declares (lz_kernels.h:165-174) for nProd
// producers and nCons consumers.  As in the kernel the level-30 producers run without the lane forms (lz_kernels.h:184) and a
// mailbox has 32 words while they hold every buffer (QN, lz_kernels.h:166).
extern "C" int emul_compress_split_ragged(const void* src, int nBlocks, int blockSize, int lastBlockSize, const unsigned* srcSizes, void* dst,
                                          int dstStride, unsigned* sizes, int level, int nProd, int nCons, int activeProd, unsigned seed)
{
    const u32 nBufs = 2u + (seed & 1u), qn = (u32)nProd * nBufs <= 32u ? 32u : 64u;
    if ((level != 10 && level != 30) || nProd < 1 || nCons < 1 || (u32)nProd * nBufs > qn) return -1;
    const bool huf = level >= 30;
    LzSplitArgs a;
    a.src = (const u8*)src; a.blockSize = (u64)blockSize; a.nBlocks = (u32)nBlocks; a.lastBlockSize = (u32)lastBlockSize;
    a.srcSizes = srcSizes; a.srcOffsets = nullptr; a.activeProd = activeProd > 0 ? (u32)activeProd : 0xFFFFFFFFu;
    a.dst = (u8*)dst; a.dstStride = (u64)dstStride; a.sizes = sizes; a.level = (u32)level;
    a.counter = (u32*)exact_area(4, 0);
    // the workgroup's share of the scratch arena: the kernel claims LZ_SPLIT_ARENA_BYTES of it (static_assert, lz_kernels.h:168)
    a.arena = (u8*)exact_area(LZ_SPLIT_ARENA_BYTES((size_t)nProd, (size_t)nCons, nBufs), 0xC7);
    a.nProd = (u32)nProd; a.nCons = (u32)nCons; a.nBufs = nBufs; a.qn = qn;
    u32* const shared = (u32*)exact_area(4u * LZ_SPLIT_SHARED_WORDS((u32)nProd, (u32)nCons, qn), 0xA5);      // shared[LZ_SPLIT_SHARED_WORDS] (lz_kernels.h:174)
    const LzSplitShared sh = lz_split_shared(shared, (u32)nProd, (u32)nCons);
    std::vector<SplitWave> waves((size_t)(nProd + nCons));
    for (int w = 0; w < nProd + nCons; w++) {
        SplitWave& x = waves[(size_t)w];
        x.a = a; x.sh = sh; x.wave = (u32)w; x.huf = huf;
        // tables[NP][kTabWords], kTabWords = LZ_TAB_BYTES(12) / 4 + 1 (lz_kernels.h:170-171); rings[NP][LZ_SEQ_RING] (:172);
        // hufWs[NC][LZ_HUF_WS_WORDS], one word each without the Huffman stage (:173)
        x.table = w < nProd ? exact_area(4u * (LZ_TAB_BYTES(12) / 4u + 1u), 0x5A) : nullptr;
        x.ring = w < nProd ? (u64*)exact_area(8u * LZ_SEQ_RING, 0xEE) : nullptr;
        x.hufWs = w >= nProd ? (u32*)exact_area(4u * (huf ? LZ_HUF_WS_WORDS : 1u), 0x77) : nullptr;
    }
    lzemu::run_wave(entry_split_init, &waves[0], seed);
    std::vector<std::thread> th;
    for (int w = 0; w < nProd + nCons; w++) th.emplace_back([&waves, w, seed] { lzemu::run_wave(entry_split_exact, &waves[(size_t)w], seed * 31u + (unsigned)w + 1u); });
    for (auto& t : th) t.join();
    for (SplitWave& x : waves) { free(x.table); free(x.ring); free(x.hufWs); }
    free(a.arena); free(shared); free(a.counter);
    return 0;
}
#endif  /* LZ_EMUL_EXACT_AREAS */
