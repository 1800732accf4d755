// lizard_gpu.hip — gfx950 kernels + the thin extern "C" shim the host C layer (lizard_host.c) calls.
//
// The kernels live in lz_kernels.h (one wavefront per Lizard API block, a persistent grid of one workgroup per CU).
// This file is the HIP side of the host layer: one context PER DEVICE (arenas, tables, streams), a per-thread device selection
// and error text, the launcher (kLevels: what a level runs; launch(): validate, look the row up, pick_arena, the row's tables, grid,
// enqueue_on), the device-buffer entry points, the shim the host C files call (lizard_gpu_ctx.h:
// lizard_pipeline_host.c holds the pipelined host-buffer path, in C), and the single-process multi-device entry with an RCCL
// all-gather of the per-block sizes (lizard_shard.h).
#include <hip/hip_runtime.h>
#include <atomic>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_shim.h"
#include "lizard_gpu_ctx.h"
#include "lz_kernels.h"   // LzBatch / LzUnBatch, residency knobs, the kernels
#include "unframe_kernels.h"   // lz_unframe_kernel: the block records of a frame (LizardGPU_decompressFrame)
#include "unframe_walk.h"      // lz_unframe_walk_kernel: the walk over a frame in device memory (LizardGPU_decompressFrame_device)
#include "lz_frame_pack.h"     // lz_frame_scan_kernel / lz_frame_gather_kernel: a frame assembled in device memory (LizardGPU_compressFrame_device)
#include "lz_frames_pack.h"    // the same for a batch of frames, and their checksums (LizardGPU_compressFrames_device)
#include "lz_stream_pack.h"    // the same for a batch of frames back to back in one buffer (LizardGPU_compressStream_device)
#include "unframes_kernels.h"  // a batch of frames walked, decoded and settled in device memory (LizardGPU_decompressFrames_device)
#include "unstream_kernels.h"  // the walk across the frames of a stream in device memory (LizardGPU_decompressStream_device)
#include "planes_kernels.h"    // the bytes of a batch of buffers split into planes and joined again (LizardGPU_splitPlanes_device)
#include "bitplanes_kernels.h" // ... and their bits (LizardGPU_splitBitPlanes_device)
#include "unslice_kernels.h"   // the records that cover byte ranges of a batch of frames (LizardGPU_decompressFrameRanges_device)
#include "planes_range_kernels.h" // an element range joined out of pieces of its planes (LizardGPU_joinPlanesRange_device)

namespace {

typedef LzStage Stage;                                 // lizard_gpu_ctx.h (plain C: shared with lizard_pipeline_host.c)
typedef LzCtx Ctx;
Ctx g_ctx[LZ_MAX_DEVICES];
struct CtxDefaults {                                   // (the contexts are zero-initialised statics; these fields start elsewhere)
    CtxDefaults() { for (Ctx& c : g_ctx) { pthread_mutex_init(&c.mu, nullptr); pthread_mutex_init(&c.comb.mu, nullptr); pthread_cond_init(&c.comb.cv, nullptr);
                                           c.device = -1; c.laneOrderOk = 1; c.hostKernelMs = -1.0f; } }
} g_ctx_defaults;
int g_default_device = 0;                              // process default (the last LizardGPU_setDevice of any thread)
pthread_mutex_t g_sel_mu = PTHREAD_MUTEX_INITIALIZER;
thread_local int  t_device = -1;                       // calling thread's selection, -1 = process default
thread_local char t_err[LZK_ERR_BYTES] = {0};

void set_err(const char* fmt, const char* a, const char* b)
{
    snprintf(t_err, sizeof t_err, fmt, a, b);
}

#define LZ_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            set_err("%s failed: %s", #call, hipGetErrorString(e_));                                    \
            return e_ == hipErrorOutOfMemory ? -LIZARDGPU_ERR_NOMEM : -LIZARDGPU_ERR_HIP;              \
        }                                                                                              \
    } while (0)

// Memory budget (LizardGPU_setMemoryBudget): bytes of device memory the large buffers of ONE device's context may take (scratch
// arenas, per-wave tables, hashChain work areas, the staging of the host-buffer entries); 0 = no cap.
std::atomic<size_t> g_budget{0};                              // read by every device's launches under their own locks, and without a lock by the getters
size_t budget_room(const Ctx& c) { const size_t b = g_budget.load(std::memory_order_relaxed); return !b ? (size_t)-1 : (b > c.devBytes ? b - c.devBytes : 0); }
int dev_alloc(Ctx& c, void** p, size_t bytes, const char* what)
{
    if (bytes > budget_room(c)) {
        snprintf(t_err, sizeof t_err, "%s: %zu bytes do not fit the memory budget of %zu bytes (%zu in use; LizardGPU_setMemoryBudget)", what, bytes, g_budget.load(), c.devBytes);
        return -LIZARDGPU_ERR_NOMEM;
    }
    LZ_HIP(hipMalloc(p, bytes));
    c.devBytes += bytes;
    return 0;
}
void dev_free(Ctx& c, void* p, size_t bytes)
{
    if (!p) return;
    (void)hipFree(p);
    c.devBytes -= bytes < c.devBytes ? bytes : c.devBytes;
}
const size_t kScratchBytes = (size_t)LZ_MAX_WAVES * LZ_SCRATCH_BYTES;     // per CU

int selected_device()
{
    if (t_device >= 0) return t_device;
    pthread_mutex_lock(&g_sel_mu);
    const int d = g_default_device;
    pthread_mutex_unlock(&g_sel_mu);
    return d;
}

// Locks the selected device's context and makes that device current for the calling thread (HIP's current device
// is per thread); restores the caller's device on exit.  (lzk_guard_acquire / _release: the same for the C files.)
void guard_acquire(LzGuard& g)
{
    g.c = nullptr; g.saved = -1; g.rc = 0;
    t_err[0] = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        snprintf(t_err, sizeof t_err, "no HIP device visible");
        g.rc = -LIZARDGPU_ERR_NO_DEVICE; return;
    }
    const int dev = selected_device();
    if (dev < 0 || dev >= count || dev >= LZ_MAX_DEVICES) {
        snprintf(t_err, sizeof t_err, "device %d out of range (%d visible)", dev, count);
        g.rc = -LIZARDGPU_ERR_ARG; return;
    }
    if (hipGetDevice(&g.saved) != hipSuccess) g.saved = -1;
    g.c = &g_ctx[dev];
    pthread_mutex_lock(&g.c->mu);
    if (hipSetDevice(dev) != hipSuccess) {
        snprintf(t_err, sizeof t_err, "hipSetDevice(%d) failed", dev); g.rc = -LIZARDGPU_ERR_HIP;
        pthread_mutex_unlock(&g.c->mu); g.c = nullptr;
        if (g.saved >= 0) (void)hipSetDevice(g.saved);
        g.saved = -1;
        return;
    }
    g.c->device = dev;
}
void guard_release(LzGuard& g)
{
    if (g.c) pthread_mutex_unlock(&g.c->mu);
    if (g.saved >= 0) (void)hipSetDevice(g.saved);
    g.c = nullptr; g.saved = -1;
}
struct Guard : LzGuard {
    Guard() { guard_acquire(*this); }
    ~Guard() { guard_release(*this); }
};

// An arena (lizard_gpu_ctx.h, LzArena): scratch, block counter and the events around its last launch; its per-wave tables come
// on first use (alloc_table_slots).  A failed arena_create leaves what it got for arena_destroy.
enum TableClass { kWide18 = 0, kPf64k = 1, kHashChain, kNoTables };   // the first LZ_ARENA_TABLES index LzArena::tables; the hashChain work areas are the context's
const size_t kTableStride[LZ_ARENA_TABLES] = { LZ_TABWIDE_BYTES(18), LZ_PF_SLOT_BYTES };
const char* const kTableWhat[LZ_ARENA_TABLES] = { "tables of levels 11/31/22/42", "tables of levels 20/40/21/41" };

int arena_create(Ctx& c, LzArena& x)
{
    memset(&x, 0, sizeof x);
    const int rc = dev_alloc(c, (void**)&x.scratch, (size_t)c.cus * kScratchBytes, "scratch arena");   // one slot per resident wave (one workgroup per CU)
    if (rc) return rc;
    LZ_HIP(hipMalloc((void**)&x.counter, 64));
    LZ_HIP(hipEventCreate(&x.ev0));
    LZ_HIP(hipEventCreate(&x.ev1));
    return 0;
}
void arena_free_tables(Ctx& c, LzArena& x, int keep)
{
    for (int k = 0; k < LZ_ARENA_TABLES; k++)
        if (k != keep) { dev_free(c, x.tables[k], x.tableSlots[k] * kTableStride[k]); x.tables[k] = nullptr; x.tableSlots[k] = 0; }
}
void arena_destroy(Ctx& c, LzArena& x)                          // (its launches have finished: caller's business)
{
    if (c.lastEv0 == x.ev0 || c.lastEv1 == x.ev1) { c.lastEv0 = c.arena[0].ev0; c.lastEv1 = c.arena[0].ev1; }      // (LizardGPU_lastKernelMs must not look at destroyed events)
    dev_free(c, x.scratch, (size_t)c.cus * kScratchBytes);
    if (x.counter) (void)hipFree(x.counter);
    arena_free_tables(c, x, kNoTables);
    if (x.ev0) (void)hipEventDestroy(x.ev0);
    if (x.ev1) (void)hipEventDestroy(x.ev1);
    memset(&x, 0, sizeof x);
}

int ctx_init_body(Ctx& c)
{
    hipDeviceProp_t prop;
    LZ_HIP(hipGetDeviceProperties(&prop, c.device));
    c.cus = prop.multiProcessorCount;
    LzArena& own = c.arena[0];
    { const int rc_ = arena_create(c, own); if (rc_) return rc_; }
#ifdef LZ_PROFILE
    LZ_HIP(hipMemset(own.scratch, 0, (size_t)c.cus * kScratchBytes));
#endif
    c.nArenas = 1; c.nextExtra = 0; c.maxArenas = LZ_ARENAS_MAX; c.lastEv0 = own.ev0; c.lastEv1 = own.ev1;
    if (const char* e = getenv("LIZARDGPU_ARENAS")) { const int n = atoi(e); if (n >= 1 && n <= LZ_ARENAS_MAX) c.maxArenas = n; }
    for (Stage& s : c.stage) {
        LZ_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        LZ_HIP(hipEventCreate(&s.k0)); LZ_HIP(hipEventCreate(&s.k1));
        LZ_HIP(hipEventCreateWithFlags(&s.meta, hipEventDisableTiming));
        LZ_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        LZ_HIP(hipEventCreateWithFlags(&s.up, hipEventDisableTiming));
    }
    // Self-check of the hardware property the exchange round (levels 10/30) and the hashChain build rely on.  A device that
    // fails it keeps working for the other levels; the dependent ones are refused, loudly (launch()).
    // LIZARDGPU_FORCE_LANE_ORDER_FAILURE=1 takes the failure branch on a healthy device (tests).
    {
        LZ_HIP(hipMemset(own.counter, 0, 4));
        hipLaunchKernelGGL(lz_selfcheck_lane_order_kernel, dim3(16), dim3(64), 0, 0, own.counter, 256u);
        LZ_HIP(hipGetLastError());
        u32 bad = 0;
        LZ_HIP(hipMemcpy(&bad, own.counter, 4, hipMemcpyDeviceToHost));
        const char* force = getenv("LIZARDGPU_FORCE_LANE_ORDER_FAILURE");
        c.laneOrderOk = bad == 0 && !(force && force[0] == '1');
        if (!c.laneOrderOk)
            fprintf(stderr, "liblizard_amd: device %d: lanes of one LDS atomic are NOT served in lane order (%u violations%s); "
                            "levels 10, 30, 12-17 and 32-38 are refused on this device\n", c.device, bad, bad ? "" : ", forced by LIZARDGPU_FORCE_LANE_ORDER_FAILURE");
    }
    c.ready = true;
    return 0;
}

void free_hc_slots(Ctx& c)
{
    dev_free(c, c.hcSlots, c.hcNSlots * c.hcSlotBytes);
    c.hcSlots = nullptr; c.hcNSlots = 0; c.hcMaxBlock = 0; c.hcHasBest = 0; c.hcSlotBytes = 0;
}

void ctx_release(Ctx& c)
{
    if (!c.ready) return;
    (void)hipSetDevice(c.device);
    (void)hipDeviceSynchronize();
    for (Stage& s : c.stage) {
        if (s.h_in) (void)hipHostFree(s.h_in);
        if (s.h_out) (void)hipHostFree(s.h_out);
        if (s.h_sizes) (void)hipHostFree(s.h_sizes);
        if (s.h_offsets) (void)hipHostFree(s.h_offsets);
        if (s.d_in) (void)hipFree(s.d_in);
        if (s.d_slots) (void)hipFree(s.d_slots);
        if (s.d_packed) (void)hipFree(s.d_packed);
        if (s.d_sizes) (void)hipFree(s.d_sizes);
        if (s.d_offsets) (void)hipFree(s.d_offsets);
        if (s.d_aux) (void)hipFree(s.d_aux);
        if (s.h_aux) (void)hipHostFree(s.h_aux);
        if (s.up) (void)hipEventDestroy(s.up);
        if (s.k0) (void)hipEventDestroy(s.k0);
        if (s.k1) (void)hipEventDestroy(s.k1);
        if (s.meta) (void)hipEventDestroy(s.meta);
        if (s.done) (void)hipEventDestroy(s.done);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        memset(&s, 0, sizeof s);
    }
    lzk_combiner_free(&c);
    if (c.dfTab) (void)hipFree(c.dfTab);
    c.dfTab = nullptr; c.dfTabCap = 0;
    for (LzArena& x : c.arena) arena_destroy(c, x);             // (every slot: one that was never made, or made half, holds nulls)
    free_hc_slots(c);
    c.nArenas = 0; c.nextExtra = 0; c.lastEv0 = c.lastEv1 = nullptr; c.laneOrderOk = 1; c.ready = 0;
    c.devBytes = 0; c.idleLaunches = 0;
}

int ctx_init(Ctx& c)
{
    if (c.ready) return 0;
    const int rc = ctx_init_body(c);
    if (rc) {                                                   // a failure half way: what was taken goes back (and is no longer counted against the budget)
        c.ready = 1; ctx_release(c);
        (void)hipGetLastError();
    }
    return rc;
}

void free_extra_arenas(Ctx& c)                                   // (their launches have finished: caller's business)
{
    for (int i = 1; i < c.nArenas; i++) arena_destroy(c, c.arena[i]);
    c.nArenas = 1; c.nextExtra = 0;
}
// Everything but the context's own scratch arena: extra arenas, per-wave tables, hashChain work areas, except the tables of class
// `keep` (kNoTables: none).  The device is idle afterwards (synchronised first: other launches may still be using what is freed).
void free_tables_except(Ctx& c, TableClass keep)
{
    (void)hipDeviceSynchronize();
    free_extra_arenas(c);
    arena_free_tables(c, c.arena[0], keep);
    if (keep != kHashChain && c.hcSlots) free_hc_slots(c);
}
// Per-wave table slots of class k for arena x under the budget: as many as resident waves if they fit — the context's own arena
// after giving up what other levels left behind, if need be — else as many as fit (the waves without one leave, lz_wave_main);
// none: out of memory.
int alloc_table_slots(Ctx& c, LzArena& x, TableClass k)
{
    const size_t want = (size_t)c.cus * LZ_MAX_WAVES, stride = kTableStride[k];
    if (want * stride > budget_room(c) && &x == &c.arena[0]) free_tables_except(c, k);
    size_t slots = budget_room(c) / stride;
    if (slots > want) slots = want;
    if (!slots) { snprintf(t_err, sizeof t_err, "%s: not one table of %zu bytes fits the memory budget of %zu bytes (%zu in use)", kTableWhat[k], stride, g_budget.load(), c.devBytes); return -LIZARDGPU_ERR_NOMEM; }
    const int rc = dev_alloc(c, (void**)&x.tables[k], slots * stride, kTableWhat[k]);
    if (rc) return rc;
    x.tableSlots[k] = slots;
    return 0;
}

int clamp_level(int level)                                       // reference lizard_compress.c:303-308
{
    if (level > LIZARD_MAX_CLEVEL) level = LIZARD_MAX_CLEVEL;
    if (level < LIZARD_MIN_CLEVEL) level = LIZARD_DEFAULT_CLEVEL;
    return level;
}

// What a level runs: one row per clamped level and block-size range (the rows of a level in ascending maxBlock; the first that
// takes the block size is the one).  A level without a row is not on the GPU path.  Everything the launcher and the getters know
// about a level comes from here.
struct LevelRow {
    int    level;
    size_t maxBlock;
    void (*enqueue)(dim3 grid, dim3 block, hipStream_t stream, const LzBatch& a);
    u32    W;                 // waves of a workgroup (one workgroup per CU)
    u32    perGroup;          // of which claim blocks: W, but for the producer / consumer form
    TableClass tables;        // per-wave tables in global memory
    bool   laneOrder;         // relies on "lanes of one LDS atomic are served in lane order" (the self-check of ctx_init_body)
    bool   needBest;          // hashChain work areas with best[] (first searches decided ahead of the parse)
};
template <void (*K)(LzBatch)>
void enqueue_kernel(dim3 grid, dim3 block, hipStream_t stream, const LzBatch& a) { hipLaunchKernelGGL(K, grid, block, 0, stream, a); }
template <void (*K)(LzBatch)>                                    // the row of kernel instantiation K
constexpr LevelRow row(int level, size_t maxBlock, u32 W, u32 perGroup, TableClass tables, bool laneOrder = false, bool needBest = false)
{
    return { level, maxBlock, enqueue_kernel<K>, W, perGroup, tables, laneOrder, needBest };
}

// The table forms of the fast and priceFast parsers keep positions modulo a power of two and sweep (lz_block.h, lz_pricefast.h): any
// size the reference takes (lib/lizard_compress.h:121).  hashChain keeps full positions; its work areas grow with the block.
const size_t kAnyBlock = (size_t)LIZARD_MAX_INPUT_SIZE;
// hashChain (13-17 / 34-38) and noChain (12 / 32 / 33: the same kernels with one candidate per search, lz_hashchain.h).  The
// arbitration follows the template argument, searchNum the run-time level: the two are tied here.
template <int LEVEL, int SEARCHLEN, int HLOG = 18>
constexpr LevelRow hc_row()
{
    constexpr bool HUF = LEVEL >= 30;
    constexpr int lv = LEVEL >= 32 ? LEVEL - 21 : LEVEL;         // 33 .. 38 are the twins of 12 .. 17; 32 is noChain too
    static_assert(SEARCHLEN == (lv <= 12 ? 6 : lv <= 15 ? lv - 6 : 4), "noChain levels 12/32/33 run <*, 6>, levels 13/14/15 and twins <*, 7/8/9>, the rest <*, 4>");
    return row<lz_hashchain_kernel<HUF, SEARCHLEN, HLOG>>(LEVEL, kAnyBlock, LZ_WAVES_HC, LZ_WAVES_HC, kHashChain, true, lv >= 16);
}
static_assert(LZ_PF_SLOT_BYTES >= (4u << 14), "levels 20/40 keep 2^14 u32 slots per wave in the 64 KiB slots of levels 21/41");
const LevelRow kLevels[] = {
#if LZ_FAST12_SPLIT                                              // (the producer / consumer form keeps every table in LDS)
    row<lz_fast12_split_kernel<false>>(10, kAnyBlock, LZ_SPLIT_PROD + LZ_SPLIT_CONS, LZ_SPLIT_PROD, kNoTables, true),
    row<lz_fast12_split_kernel<true>>(30, kAnyBlock, LZ_SPLIT_PROD_HUF + LZ_SPLIT_CONS_HUF, LZ_SPLIT_PROD_HUF, kNoTables, true),
#else                                                            // (tuning builds; global-table waves hold 22-bit positions: blocks up to 4 MiB)
    row<lz_fast12_kernel<false, true>>(10, 4u << 20, LZ_WAVES_FAST, LZ_WAVES_FAST, kPf64k, true),
    row<lz_fast12_kernel<false, false>>(10, kAnyBlock, LZ_WAVES_FASTLDS, LZ_WAVES_FASTLDS, kPf64k, true),
    row<lz_fast12_kernel<true, true>>(30, 4u << 20, LZ_WAVES_FAST_HUF, LZ_WAVES_FAST_HUF, kPf64k, true),
    row<lz_fast12_kernel<true, false>>(30, kAnyBlock, LZ_WAVES_FASTLDS_HUF, LZ_WAVES_FASTLDS_HUF, kPf64k, true),
#endif
    row<lz_fast18_kernel<false>>(11, kAnyBlock, LZ_WAVES_FAST18, LZ_WAVES_FAST18, kWide18),
    row<lz_fast18_kernel<true>>(31, kAnyBlock, LZ_WAVES_FAST18, LZ_WAVES_FAST18, kWide18),
    hc_row<12, 6>(), hc_row<13, 7>(), hc_row<14, 8>(), hc_row<15, 9>(), hc_row<16, 4>(), hc_row<17, 4>(),
    hc_row<32, 6, 14>(), hc_row<33, 6>(), hc_row<34, 7>(), hc_row<35, 8>(), hc_row<36, 9>(), hc_row<37, 4>(), hc_row<38, 4>(),
    row<lz_fastbig14_kernel<false>>(20, kAnyBlock, LZ_WAVES_FASTBIG, LZ_WAVES_FASTBIG, kPf64k),
    row<lz_fastbig14_kernel<true>>(40, kAnyBlock, LZ_WAVES_FASTBIG, LZ_WAVES_FASTBIG, kPf64k),
    row<lz_pricefast18_kernel<false>>(22, kAnyBlock, LZ_PF22_W, LZ_PF22_W, kWide18),
    row<lz_pricefast18_kernel<true>>(42, kAnyBlock, LZ_PF22_W, LZ_PF22_W, kWide18),
    row<lz_pricefast14_kernel<false, true>>(21, 256u << 10, LZ_PF18_W, LZ_PF18_W, kPf64k),      // 18-bit LDS tables
    row<lz_pricefast14_kernel<false, false>>(21, kAnyBlock, LZ_PF_W, LZ_PF_W, kPf64k),
    row<lz_pricefast14_kernel<true, true>>(41, 256u << 10, LZ_PF18_W_HUF, LZ_PF18_W_HUF, kPf64k),
    row<lz_pricefast14_kernel<true, false>>(41, kAnyBlock, LZ_PF_W, LZ_PF_W, kPf64k),
};
const LevelRow* find_row(int lv, size_t blockSize)
{
    for (const LevelRow& r : kLevels) if (r.level == lv && blockSize <= r.maxBlock) return &r;
    return nullptr;
}
// Largest block the GPU path takes at a level (0 = level not on the GPU path).
size_t level_max_block(int lv)
{
    size_t m = 0;
    for (const LevelRow& r : kLevels) if (r.level == lv && r.maxBlock > m) m = r.maxBlock;
    return m;
}

// Which arena?  (lizard_gpu_ctx.h, LzArena.)  The context's own unless this is a small launch (`eligible`: fewer blocks than the
// machine has claiming waves, not hashChain) on another stream than the one that used it last and that launch is still running;
// then: an extra arena last used by this stream, or an idle one, or a new one, or — all busy, none left to make — the extra ones
// in turn.
LzArena* pick_arena(Ctx& c, bool eligible, hipStream_t stream)
{
    LzArena& own = c.arena[0];
    LzArena* ar = nullptr;
    if (eligible && c.maxArenas > 1 && own.timed && own.lastStream != stream && hipEventQuery(own.ev1) != hipSuccess) {
        for (int i = 1; i < c.nArenas && !ar; i++) if (c.arena[i].lastStream == stream) ar = &c.arena[i];
        for (int i = 1; i < c.nArenas && !ar; i++) if (!c.arena[i].timed || hipEventQuery(c.arena[i].ev1) == hipSuccess) ar = &c.arena[i];   // (anything but success: busy)
        if (!ar && c.nArenas < c.maxArenas && budget_room(c) >= (size_t)c.cus * kScratchBytes) {
            LzArena& x = c.arena[c.nArenas];
            if (arena_create(c, x) == 0) {
                ar = &x; c.nArenas++;
                if (getenv("LIZARDGPU_VERBOSE")) fprintf(stderr, "liblizard_amd: device %d: arena %d for small launches on concurrent streams (LIZARDGPU_ARENAS caps them)\n", c.device, c.nArenas);
            } else { arena_destroy(c, x); t_err[0] = 0; }        // no room: share the context's own after all
        }
        if (!ar && c.nArenas > 1) { ar = &c.arena[1 + c.nextExtra % (c.nArenas - 1)]; c.nextExtra++; }
        (void)hipGetLastError();                                 // (hipEventQuery's "not ready" is not an error to report)
    }
    // extra arenas that no launch has asked for in a while go back (64 launches on the context's own arena, all of theirs finished)
    if (ar) { c.idleLaunches = 0; return ar; }
    if (c.nArenas > 1 && eligible && ++c.idleLaunches >= 64) {   // (launches that could have asked for one: large and hashChain launches say nothing about the small streams)
        bool idle = true;
        for (int i = 1; i < c.nArenas; i++) if (c.arena[i].timed && hipEventQuery(c.arena[i].ev1) != hipSuccess) idle = false;
        (void)hipGetLastError();
        if (idle) free_extra_arenas(c);
        c.idleLaunches = 0;
    }
    return &own;
}

// The per-wave tables of class k in *ar, allocated on first use.  An extra arena whose tables do not fit the memory budget any
// more (the hashChain work areas or the context's own tables took the room): the launch goes to the context's own arena after
// all — it waits for the launch that holds it, and may give up what other levels left behind — instead of failing where it
// would have succeeded on a quiet device.
int ensure_arena_tables(Ctx& c, LzArena*& ar, TableClass k)
{
    if (!ar->tables[k] && ar != &c.arena[0] && alloc_table_slots(c, *ar, k)) { (void)hipGetLastError(); ar = &c.arena[0]; }
    return ar->tables[k] ? 0 : alloc_table_slots(c, *ar, k);
}

// The hashChain work areas (the context's, not an arena's).  Per wave: bins, links, and 6 bytes + 1 bit per block position (chain,
// packed chain words, hit bits) — 10 bytes at levels 16/17/37/38, whose first searches are decided ahead of the parse (best[],
// the LAST array of the slot: the other levels' slots simply end before it).  One slot per resident wave while that fits in
// about half of the free memory (256 KiB blocks: 14 GiB, 18 GiB with best[]; 4 MiB blocks: 110 GiB, or as many slots as fit under
// the 128 GiB cap with best[]); larger blocks get as many slots as fit and the other waves leave (lz_wave_main).
int ensure_hc_slots(Ctx& c, int lv, size_t blockSize, bool needBest)
{
    const size_t cap = (blockSize + 65535u) & ~(size_t)65535u;
    if (c.hcSlots && c.hcMaxBlock >= cap && (!needBest || c.hcHasBest)) return 0;
    const bool withBest = needBest || c.hcHasBest;
    const size_t capA = cap > c.hcMaxBlock ? cap : c.hcMaxBlock;                 // (a re-allocation never shrinks what the slots take)
    const size_t slotBytes = LZ_HC_SLOT_BYTES(capA) - (withBest ? 0u : 4u * capA);
    if (c.hcSlots) { LZ_HIP(hipDeviceSynchronize()); dev_free(c, c.hcSlots, c.hcNSlots * c.hcSlotBytes); c.hcSlots = nullptr; c.hcNSlots = 0; }
    size_t freeB = 0, totalB = 0;
    LZ_HIP(hipMemGetInfo(&freeB, &totalB));
    size_t budget = freeB / 2u;
    if (budget > ((size_t)128 << 30)) budget = (size_t)128 << 30;
    if (g_budget.load(std::memory_order_relaxed)) {      // LizardGPU_setMemoryBudget: what other levels left behind goes first
        if (budget_room(c) < (size_t)c.cus * LZ_MAX_WAVES * slotBytes) free_tables_except(c, kHashChain);
        if (budget > budget_room(c)) budget = budget_room(c);
    }
    // LIZARDGPU_HC_WORKAREA_MB caps the reservation (a caller that shares the device with other allocations); fewer work
    // areas than resident waves only means fewer hashChain blocks in flight (the waves without one leave)
    if (const char* e = getenv("LIZARDGPU_HC_WORKAREA_MB")) {
        const size_t mb = (size_t)strtoull(e, nullptr, 10);
        if (mb > 0 && (mb << 20) < budget) budget = mb << 20;
    }
    size_t nSlots = budget / slotBytes;
    if (nSlots > (size_t)c.cus * LZ_MAX_WAVES) nSlots = (size_t)c.cus * LZ_MAX_WAVES;
    if (nSlots == 0) { snprintf(t_err, sizeof t_err, "level %d: no room for a hashChain work area of %zu bytes", lv, slotBytes); return -LIZARDGPU_ERR_NOMEM; }
    { const int rc_ = dev_alloc(c, (void**)&c.hcSlots, nSlots * slotBytes, "hashChain work areas"); if (rc_) return rc_; }
    c.hcMaxBlock = capA; c.hcNSlots = nSlots; c.hcHasBest = withBest; c.hcSlotBytes = slotBytes;
    if (getenv("LIZARDGPU_VERBOSE"))
        fprintf(stderr, "liblizard_amd: device %d: hashChain levels reserve %zu work areas of %zu bytes (%.1f GiB of %.1f GiB free; LIZARDGPU_HC_WORKAREA_MB caps it)\n",
                c.device, nSlots, slotBytes, (double)(nSlots * slotBytes) / (double)(1u << 30), (double)freeB / (double)(1u << 30));
    return 0;
}

// One kernel on arena x.  The scratch arena, the tables and the block counter of an arena are shared by all its launches: a
// launch on another stream first waits (on the GPU) for the previous one to finish (always, also on the stream that used the
// arena last: a destroyed stream's handle can come back for a new stream, and a same-stream wait costs nothing).  k0 / k1 (may be
// null) are recorded around the kernel.
template <class Launch>
int enqueue_on(Ctx& c, LzArena& x, hipStream_t stream, hipEvent_t k0, hipEvent_t k1, Launch launchKernel)
{
    if (x.timed) LZ_HIP(hipStreamWaitEvent(stream, x.ev1, 0));
    LZ_HIP(hipMemsetAsync(x.counter, 0, 4, stream));
    LZ_HIP(hipEventRecord(x.ev0, stream));
    if (k0) LZ_HIP(hipEventRecord(k0, stream));
    launchKernel();
    LZ_HIP(hipGetLastError());
    LZ_HIP(hipEventRecord(x.ev1, stream));
    if (k1) LZ_HIP(hipEventRecord(k1, stream));
    x.timed = 1; x.lastStream = stream;
    c.lastEv0 = x.ev0; c.lastEv1 = x.ev1;
    return 0;
}

// d_srcSizes / d_srcOffsets (may be nullptr, both or neither): a ragged batch — block b is d_srcSizes[b] bytes (1..blockSize) at
// d_src + d_srcOffsets[b]; lastBlockSize is ignored then (pass blockSize).
int launch(Ctx& c, const void* d_src, size_t nBlocks, size_t blockSize, size_t lastBlockSize, void* d_dst,
           size_t dstStride, u32* d_sizes, int level, hipStream_t stream, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr,
           const u32* d_srcSizes = nullptr, const u64* d_srcOffsets = nullptr)
{
    const int lv = clamp_level(level);
    if (!level_max_block(lv)) { snprintf(t_err, sizeof t_err, "level %d has no GPU kernel", lv); return -LIZARDGPU_ERR_LEVEL; }
    if (!d_src || !d_dst || !d_sizes || nBlocks == 0 || nBlocks > 0xFFFFFFFFu || blockSize == 0 || blockSize > LIZARD_MAX_INPUT_SIZE
        || lastBlockSize == 0 || lastBlockSize > blockSize || dstStride < (size_t)LIZARD_COMPRESSBOUND((int)blockSize)) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer, zero size, lastBlockSize > blockSize or dstStride < Lizard_compressBound)");
        return -LIZARDGPU_ERR_ARG;
    }
    const LevelRow* const row = find_row(lv, blockSize);
    if (!row) {
        snprintf(t_err, sizeof t_err, "level %d: blocks above %zu bytes are not supported on the GPU path", lv, level_max_block(lv));
        return -LIZARDGPU_ERR_ARG;
    }
    int rc = ctx_init(c);
    if (rc) return rc;
    if (!c.laneOrderOk && row->laneOrder) {
        snprintf(t_err, sizeof t_err, "level %d refused: device %d failed the self-check \"lanes of one LDS atomic are served in lane order\" its kernel relies on", lv, c.device);
        return -LIZARDGPU_ERR_HARDWARE;
    }
    const bool smallLaunch = nBlocks < (size_t)c.cus * row->perGroup;
    LzArena* ar = pick_arena(c, smallLaunch && row->tables != kHashChain, stream);
    LzBatch a;
    a.src = (const u8*)d_src; a.blockSize = blockSize; a.nBlocks = (u32)nBlocks; a.lastBlockSize = (u32)lastBlockSize;
    a.dst = (u8*)d_dst; a.dstStride = dstStride; a.sizes = d_sizes; a.level = (u32)lv;
    a.tables = nullptr; a.tableStride = 0; a.tableSlots = 0xFFFFFFFFu;
    a.srcSizes = d_srcSizes; a.srcOffsets = d_srcOffsets; a.activeWaves = 0xFFFFFFFFu;
    if (row->tables == kHashChain) {
        if ((rc = ensure_hc_slots(c, lv, blockSize, row->needBest))) return rc;
        a.tables = c.hcSlots; a.tableStride = c.hcSlotBytes; a.tableSlots = (u32)c.hcNSlots;
    } else if (row->tables != kNoTables) {
        const TableClass k = row->tables;
        if ((rc = ensure_arena_tables(c, ar, k))) return rc;
        a.tables = ar->tables[k]; a.tableStride = kTableStride[k]; a.tableSlots = (u32)ar->tableSlots[k];
    }
    a.scratch = ar->scratch; a.counter = ar->counter;
    // one workgroup of W waves per CU; small batches launch only as many workgroups as they have blocks for
    u32 grid = (u32)((nBlocks + row->perGroup - 1) / row->perGroup);
    if (grid > (u32)c.cus) grid = (u32)c.cus;
#if LZ_SPREAD_SMALL
    // A launch with fewer blocks than the chip has block-claiming waves is spread over ALL CUs, ceil(nBlocks / grid) claiming
    // waves per workgroup, instead of filling nBlocks / perGroup CUs to the brim: 256 blocks are 256 CUs x 1 wave, not 20 x 13.
    if (smallLaunch) {
        grid = nBlocks < (size_t)c.cus ? (u32)nBlocks : (u32)c.cus;
        a.activeWaves = (u32)((nBlocks + grid - 1) / grid);
    }
#endif
    rc = enqueue_on(c, *ar, stream, k0, k1, [&] { row->enqueue(dim3(grid), dim3(64 * row->W), stream, a); });
    if (!rc) c.lastSplit = row->perGroup != row->W;              // (only the producer / consumer form has waves that claim no block)
    return rc;
}

// What the four decode launchers share behind their own argument check and struct fill: the context's own arena (its scratch and
// counter are shared with the compress launches, ordered by the same events) into the kernel's arguments, one wave per item on a
// persistent grid of at most one workgroup per CU (lz_decode_grid, lz_kernels.h).
template <class Batch>
int launch_decode_grid(Ctx& c, void (*kernel)(Batch), Batch& a, size_t nItems, hipStream_t stream)
{
    int rc = ctx_init(c);
    if (rc) return rc;
    LzArena& own = c.arena[0];
    a.scratch = own.scratch; a.counter = own.counter;
    u32 grid = (u32)((nItems + LZ_WAVES_DEC - 1) / LZ_WAVES_DEC);
    if (grid > (u32)c.cus) grid = (u32)c.cus;
    c.hostKernelMs = -1.0f;
    return enqueue_on(c, own, stream, nullptr, nullptr, [&] { hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * LZ_WAVES_DEC), 0, stream, a); });
}

int launch_decompress(Ctx& c, const void* d_src, const u64* d_offsets, size_t srcStride, const u32* d_srcSizes, size_t nBlocks,
                      void* d_dst, size_t dstStride, u32* d_outSizes, hipStream_t stream)
{
    if (!d_src || !d_dst || !d_outSizes || (!d_offsets && !d_srcSizes) || nBlocks == 0 || nBlocks > 0xFFFFFFFFu || dstStride == 0) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or zero size)");
        return -LIZARDGPU_ERR_ARG;
    }
    LzUnBatch a;
    a.src = (const u8*)d_src; a.offsets = d_offsets; a.srcStride = srcStride; a.srcSizes = d_srcSizes;
    a.dst = (u8*)d_dst; a.dstStride = dstStride; a.outSizes = d_outSizes; a.nBlocks = (u32)nBlocks;
    return launch_decode_grid(c, lz_decompress_kernel, a, nBlocks, stream);
}

// The records of one chunk of a frame (unframe_kernels.h).
int launch_unframe(Ctx& c, const void* d_src, const u64* d_payloadOffsets, const u32* d_words, size_t nRecords, void* d_slots,
                   size_t slotBytes, u32* d_outSizes, u32* d_packSizes, hipStream_t stream)
{
    if (!d_src || !d_payloadOffsets || !d_words || !d_slots || !d_outSizes || !d_packSizes || nRecords == 0 || nRecords > 0xFFFFFFFFu || slotBytes == 0) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or zero size)");
        return -LIZARDGPU_ERR_ARG;
    }
    LzUnframeBatch a;
    a.src = (const u8*)d_src; a.payloadOffsets = d_payloadOffsets; a.words = d_words;
    a.slots = (u8*)d_slots; a.slotBytes = slotBytes; a.outSizes = d_outSizes; a.packSizes = d_packSizes; a.nRecords = (u32)nRecords;
    return launch_decode_grid(c, lz_unframe_kernel, a, nRecords, stream);
}

// The same with the slots inside the caller's buffer (lz_unframe_inplace_kernel).
int launch_unframe_inplace(Ctx& c, const void* d_src, const u64* d_payloadOffsets, const u32* d_words, size_t nRecords, void* d_dst,
                           size_t slotBytes, size_t dstRoom, u32* d_outSizes, u32* d_packSizes, hipStream_t stream)
{
    if (!d_src || !d_payloadOffsets || !d_words || !d_dst || !d_outSizes || !d_packSizes || nRecords == 0 || nRecords > 0xFFFFFFFFu || slotBytes == 0
        || dstRoom == 0 || (nRecords - 1) > (dstRoom - 1) / slotBytes) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer, zero size or a slot that starts outside the buffer)");
        return -LIZARDGPU_ERR_ARG;
    }
    LzUnframeInPlaceBatch a;
    a.src = (const u8*)d_src; a.payloadOffsets = d_payloadOffsets; a.words = d_words;
    a.dst = (u8*)d_dst; a.slotBytes = slotBytes; a.dstRoom = dstRoom; a.outSizes = d_outSizes; a.packSizes = d_packSizes; a.nRecords = (u32)nRecords;
    return launch_decode_grid(c, lz_unframe_inplace_kernel, a, nRecords, stream);
}

// One segment of the frame walk (unframe_walk.h): one wave, no arena.
int launch_walk(Ctx& c, const void* d_src, size_t srcSize, size_t startPos, size_t budget, size_t tableCap, u64* d_offs, u32* d_words,
                LzWalkResult* d_res, hipStream_t stream)
{
    if ((!d_src && srcSize) || !d_res || startPos > srcSize) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or a start behind the end)");
        return -LIZARDGPU_ERR_ARG;
    }
    int rc = ctx_init(c);
    if (rc) return rc;
    LzWalkArgs a;
    a.src = (const u8*)d_src; a.srcSize = srcSize; a.startPos = startPos; a.budget = budget; a.tableCap = tableCap;
    a.offs = d_offs; a.words = d_words; a.res = d_res;
    hipLaunchKernelGGL(lz_unframe_walk_kernel, dim3(1), dim3(64), 0, stream, a);
    LZ_HIP(hipGetLastError());
    return 0;
}

// All records of a batch of frames, each decoded in place in its own frame's buffer (unframes_kernels.h).
int launch_unframes(Ctx& c, const LzUnframesEntry* d_frames, const u64* d_offs, const u32* d_words, const u32* d_recFrame, u32* d_out,
                    size_t nRecords, hipStream_t stream)
{
    if (!d_frames || !d_offs || !d_words || !d_recFrame || !d_out || nRecords == 0 || nRecords > 0xFFFFFFFFu) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or no records)");
        return -LIZARDGPU_ERR_ARG;
    }
    LzUnframesBatch a;
    a.frames = d_frames; a.offs = d_offs; a.words = d_words; a.recFrame = d_recFrame; a.out = d_out; a.nRecords = (u32)nRecords;
    return launch_decode_grid(c, lz_unframes_kernel, a, nRecords, stream);
}

// The picked records of a batch of frames, each into its slot in ONE destination (unslice_kernels.h).
int launch_unslice(Ctx& c, const LzUnframesEntry* d_frames, const u64* d_offs, const u32* d_words, const LzSlicePick* d_picks, void* d_dst,
                   u32* d_out, size_t nPicks, hipStream_t stream)
{
    if (!d_frames || !d_offs || !d_words || !d_picks || !d_dst || !d_out || nPicks == 0 || nPicks > 0xFFFFFFFFu) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or no picks)");
        return -LIZARDGPU_ERR_ARG;
    }
    LzUnsliceBatch a;
    a.frames = d_frames; a.offs = d_offs; a.words = d_words; a.picks = d_picks; a.dst = (u8*)d_dst; a.out = d_out; a.nPicks = (u32)nPicks;
    return launch_decode_grid(c, lz_unslice_kernel, a, nPicks, stream);
}

}  // namespace

#include "lizard_shard.h"   // single-process multi-device entry + RCCL size gather (uses Guard / launch above)

extern "C" {

int LizardGPU_levelSupported(int level)
{
    return level_max_block(clamp_level(level)) != 0;
}

size_t LizardGPU_maxBlockSize(int level) { return level_max_block(clamp_level(level)); }

int LizardGPU_deviceCount(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return count;
}

int LizardGPU_setDevice(int device)
{
    t_err[0] = 0;
    const int count = LizardGPU_deviceCount();
    if (device < 0 || device >= LZ_MAX_DEVICES || (count > 0 && device >= count)) {
        snprintf(t_err, sizeof t_err, "LizardGPU_setDevice(%d): %d device(s) visible", device, count);
        return -LIZARDGPU_ERR_ARG;
    }
    t_device = device;
    pthread_mutex_lock(&g_sel_mu);
    g_default_device = device;
    pthread_mutex_unlock(&g_sel_mu);
    return 0;
}

const char* LizardGPU_lastError(void) { return t_err; }

int LizardGPU_residentWaves(void)
{
    Guard g;
    if (g.rc) return g.rc;
    int rc = ctx_init(*g.c);
    return rc ? rc : g.c->cus * (int)find_row(10, 1)->perGroup;      // level-10 residency: blocks in flight = waves with a hash table (13 per CU, all in LDS)
}

static void release_all_contexts(size_t newBudget, bool setBudget)
{
    int saved = -1;
    if (hipGetDevice(&saved) != hipSuccess) saved = -1;
    // every context is quiesced and locked BEFORE the budget changes, and released under the new one: no launch on any device
    // runs with holdings counted against the old budget while it reads the new (round 5 stored it under context 0's lock alone)
    for (int d = 0; d < LZ_MAX_DEVICES; d++) { lzk_combiner_quiesce(&g_ctx[d]); pthread_mutex_lock(&g_ctx[d].mu); }
    if (setBudget) g_budget.store(newBudget, std::memory_order_relaxed);
    for (int d = 0; d < LZ_MAX_DEVICES; d++) ctx_release(g_ctx[d]);
    for (int d = LZ_MAX_DEVICES - 1; d >= 0; d--) { pthread_mutex_unlock(&g_ctx[d].mu); lzk_combiner_resume(&g_ctx[d]); }
    if (saved >= 0) (void)hipSetDevice(saved);
}

void LizardGPU_shutdown(void)
{
    release_all_contexts(0, false);
    lz_shard_shutdown();
}

int LizardGPU_setMemoryBudget(size_t bytes)
{
    t_err[0] = 0;
    if (bytes) {
        int count = 0, cus = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) count = 0;
        for (int d = 0; d < count; d++) {                   // the budget holds for every device: the floor is the largest one's
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, d) == hipSuccess && prop.multiProcessorCount > cus) cus = prop.multiProcessorCount;
        }
        if (!cus) {
            (void)hipGetLastError();
            snprintf(t_err, sizeof t_err, "no HIP device visible");
            return -LIZARDGPU_ERR_NO_DEVICE;
        }
        const size_t floor_ = (size_t)cus * kScratchBytes + ((size_t)256 << 20);
        if (bytes < floor_) {
            snprintf(t_err, sizeof t_err, "LizardGPU_setMemoryBudget(%zu): below the minimum of %zu bytes (one scratch arena of %zu bytes + 256 MiB)", bytes, floor_, floor_ - ((size_t)256 << 20));
            return -LIZARDGPU_ERR_ARG;
        }
    }
    release_all_contexts(bytes, true);                  // what the contexts hold goes back; the next call allocates under the new budget
    return 0;
}

size_t LizardGPU_memoryBudget(void) { return g_budget.load(std::memory_order_relaxed); }

size_t LizardGPU_memoryInUse(void)
{
    Guard g;
    return g.rc ? 0 : g.c->devBytes;
}

// Give back what is idle on the selected device: extra arenas, per-wave tables, hashChain work areas, the staging buffers of the
// host-buffer entries and of the one-block combiner.  The context's own scratch arena stays.  Waits for the device to be idle.
int LizardGPU_trim(void)
{
    LzCtx* const cpeek = lzk_ctx_peek();
    if (!cpeek) return -LIZARDGPU_ERR_NO_DEVICE;
    lzk_combiner_quiesce(cpeek);
    int rc = 0;
    {
        Guard g;
        rc = g.rc;
        if (!rc && g.c->ready) {
            Ctx& c = *g.c;
            free_tables_except(c, kNoTables);
            for (Stage& s : c.stage) {
                dev_free(c, s.d_in, s.d_in_cap); dev_free(c, s.d_slots, s.d_slots_cap); dev_free(c, s.d_packed, s.d_packed_cap);
                s.d_in = s.d_slots = s.d_packed = nullptr; s.d_in_cap = s.d_slots_cap = s.d_packed_cap = 0;
                if (s.h_in) (void)hipHostFree(s.h_in);
                if (s.h_out) (void)hipHostFree(s.h_out);
                s.h_in = s.h_out = nullptr; s.h_in_cap = s.h_out_cap = 0;
            }
            dev_free(c, c.dfTab, c.dfTabCap); c.dfTab = nullptr; c.dfTabCap = 0;
            if (g.c == cpeek) lzk_combiner_free(&c);
        }
    }
    lzk_combiner_resume(cpeek);
    return rc;
}

int LizardGPU_compressBlocks_device(const void* d_src, size_t nBlocks, size_t blockSize, size_t lastBlockSize,
                                    void* d_dst, size_t dstStride, uint32_t* d_sizes, int level, void* stream)
{
    Guard g;
    if (g.rc) return g.rc;
    g.c->hostKernelMs = -1.0f;
    return launch(*g.c, d_src, nBlocks, blockSize, lastBlockSize, d_dst, dstStride, d_sizes, level, (hipStream_t)stream);
}

int LizardGPU_decompressBlocks_device(const void* d_src, size_t srcStride, const uint32_t* d_srcSizes, size_t nBlocks,
                                      void* d_dst, size_t dstStride, uint32_t* d_outSizes, void* stream)
{
    Guard g;
    if (g.rc) return g.rc;
    return launch_decompress(*g.c, d_src, nullptr, srcStride, d_srcSizes, nBlocks, d_dst, dstStride, d_outSizes, (hipStream_t)stream);
}

// ---- the shim of lizard_gpu_ctx.h: what the host C files (lizard_pipeline_host.c) need from this side ----
void  lzk_guard_acquire(LzGuard* g) { guard_acquire(*g); }
void  lzk_guard_release(LzGuard* g) { guard_release(*g); }
char* lzk_err(void) { return t_err; }
int   lzk_ctx_init(LzCtx* c) { return ctx_init(*c); }
int   lzk_clamp_level(int level) { return clamp_level(level); }
int   lzk_launch(LzCtx* c, const void* d_src, size_t nBlocks, size_t blockSize, size_t lastBlockSize, void* d_dst, size_t dstStride,
                 uint32_t* d_sizes, int level, hipStream_t stream, hipEvent_t k0, hipEvent_t k1, const uint32_t* d_srcSizes,
                 const uint64_t* d_srcOffsets)
{
    return launch(*c, d_src, nBlocks, blockSize, lastBlockSize, d_dst, dstStride, d_sizes, level, stream, k0, k1, d_srcSizes, (const u64*)d_srcOffsets);
}
int    lzk_dev_alloc(LzCtx* c, void** p, size_t bytes)
{
    // staging of a host-buffer call (context locked by the caller): under a budget, the tables and work areas earlier launches left
    // behind make room for it (this call's own launch gets as many table slots as still fit)
    if (bytes > budget_room(*c)) free_tables_except(*c, kNoTables);
    return dev_alloc(*c, p, bytes, "staging buffer");
}
void   lzk_dev_free(LzCtx* c, void* p, size_t bytes) { dev_free(*c, p, bytes); }
size_t lzk_budget(void) { return g_budget.load(std::memory_order_relaxed); }
size_t lzk_budget_room_for_staging(const LzCtx* c)
{
    const size_t b = g_budget.load(std::memory_order_relaxed), arena = (size_t)c->cus * kScratchBytes;
    return !b ? (size_t)-1 : (b > arena ? b - arena : 0);
}
LzCtx* lzk_ctx_peek(void)
{
    int count = 0;
    t_err[0] = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        snprintf(t_err, sizeof t_err, "no HIP device visible");
        return nullptr;
    }
    const int dev = selected_device();
    if (dev < 0 || dev >= count || dev >= LZ_MAX_DEVICES) { snprintf(t_err, sizeof t_err, "device %d out of range (%d visible)", dev, count); return nullptr; }
    return &g_ctx[dev];
}
int   lzk_launch_decompress(LzCtx* c, const void* d_src, const uint64_t* d_offsets, size_t srcStride, const uint32_t* d_srcSizes,
                            size_t nBlocks, void* d_dst, size_t dstStride, uint32_t* d_outSizes, hipStream_t stream)
{
    return launch_decompress(*c, d_src, (const u64*)d_offsets, srcStride, d_srcSizes, nBlocks, d_dst, dstStride, d_outSizes, stream);
}
int   lzk_launch_unframe(LzCtx* c, const void* d_src, const uint64_t* d_payloadOffsets, const uint32_t* d_words, size_t nRecords, void* d_slots,
                         size_t slotBytes, uint32_t* d_outSizes, uint32_t* d_packSizes, hipStream_t stream)
{
    return launch_unframe(*c, d_src, (const u64*)d_payloadOffsets, d_words, nRecords, d_slots, slotBytes, d_outSizes, d_packSizes, stream);
}
int   lzk_launch_walk(LzCtx* c, const void* d_src, size_t srcSize, size_t startPos, size_t budget, size_t tableCap, uint64_t* d_offs,
                      uint32_t* d_words, struct LzWalkResult* d_res, hipStream_t stream)
{
    return launch_walk(*c, d_src, srcSize, startPos, budget, tableCap, (u64*)d_offs, d_words, d_res, stream);
}
int   lzk_launch_unframe_inplace(LzCtx* c, const void* d_src, const uint64_t* d_payloadOffsets, const uint32_t* d_words, size_t nRecords,
                                 void* d_dst, size_t slotBytes, size_t dstRoom, uint32_t* d_outSizes, uint32_t* d_packSizes, hipStream_t stream)
{
    return launch_unframe_inplace(*c, d_src, (const u64*)d_payloadOffsets, d_words, nRecords, d_dst, slotBytes, dstRoom, d_outSizes, d_packSizes, stream);
}
void  lzk_pack_launch(const void* d_in, const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, void* d_packed,
                      uint32_t nb, uint32_t blockSize, uint32_t lastBlockSize, int mode, hipStream_t stream)
{
    static_assert(LZK_PACK_PAYLOAD == LZ_PACK_PAYLOAD && LZK_PACK_FRAME == LZ_PACK_FRAME, "pack modes");
    lz_pack_launch((const u8*)d_in, (const u8*)d_slots, slot, d_sizes, (u64*)d_offsets, (u8*)d_packed, nb, blockSize, lastBlockSize, mode, stream);
}
int   lzk_frame_pack_launch(const void* d_in, const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, void* d_dst,
                            uint32_t nb, uint32_t blockSize, uint32_t lastBlockSize, uint64_t* d_state, uint64_t limit, hipStream_t stream)
{
    static_assert(sizeof(LzFrameState) == 4 * sizeof(uint64_t), "the state the host reads back");
    if (!d_in || !d_slots || !d_sizes || !d_offsets || !d_dst || !d_state || nb == 0 || blockSize == 0 || lastBlockSize == 0 || lastBlockSize > blockSize) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer, no blocks or lastBlockSize > blockSize)");
        return -LIZARDGPU_ERR_ARG;
    }
    lz_frame_pack_launch((const u8*)d_in, (const u8*)d_slots, slot, d_sizes, (u64*)d_offsets, (u8*)d_dst, nb, blockSize, lastBlockSize,
                         (LzFrameState*)d_state, limit, stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_frames_pack_launch(const void* d_base, const uint64_t* d_blkOffsets, const uint32_t* d_blkSizes, const uint32_t* d_blkFrames,
                             const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, uint32_t nb,
                             LzFramesEntry* d_frames, hipStream_t stream)
{
    if (!d_base || !d_blkOffsets || !d_blkSizes || !d_blkFrames || !d_slots || !d_sizes || !d_offsets || !d_frames || nb == 0) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or no blocks)");
        return -LIZARDGPU_ERR_ARG;
    }
    lz_frames_pack_launch((const u8*)d_base, (const u64*)d_blkOffsets, d_blkSizes, d_blkFrames, (const u8*)d_slots, slot, d_sizes, (u64*)d_offsets,
                          nb, d_frames, stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_frames_hash_launch(LzFramesEntry* d_frames, uint32_t nFrames, hipStream_t stream)
{
    if (!d_frames || nFrames == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no frames)"); return -LIZARDGPU_ERR_ARG; }
    lz_frames_hash_launch(d_frames, nFrames, stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_frames_finish_launch(const LzFramesEntry* d_frames, LzFramesResult* d_results, uint32_t nFrames, hipStream_t stream)
{
    if (!d_frames || !d_results || nFrames == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no frames)"); return -LIZARDGPU_ERR_ARG; }
    lz_frames_finish_launch(d_frames, d_results, nFrames, stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_stream_pack_launch(const void* d_base, const uint64_t* d_blkOffsets, const uint32_t* d_blkSizes, const uint32_t* d_blkFrames,
                             const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, uint32_t nb, uint32_t firstBlock,
                             const LzFramesEntry* d_frames, LzStreamEntry* d_entries, LzStreamState* d_state, uint64_t capacity, hipStream_t stream)
{
    static_assert(sizeof(LzStreamEntry) == 56 && sizeof(LzStreamState) == 16, "the tables the host file fills");
    if (!d_base || !d_blkOffsets || !d_blkSizes || !d_blkFrames || !d_slots || !d_sizes || !d_offsets || !d_frames || !d_entries || !d_state || nb == 0) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or no blocks)");
        return -LIZARDGPU_ERR_ARG;
    }
    lz_stream_pack_launch((const u8*)d_base, (const u64*)d_blkOffsets, d_blkSizes, d_blkFrames, (const u8*)d_slots, slot, d_sizes, (u64*)d_offsets,
                          nb, firstBlock, d_frames, d_entries, d_state, capacity, stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_stream_finish_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const void* d_blob, const LzStreamState* d_state,
                               uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, LzFramesResult* d_result, uint64_t* d_offsets,
                               hipStream_t stream)
{
    if (!d_frames || !d_entries || !d_blob || !d_state || !d_result || !d_offsets || nFrames == 0) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or no frames)");
        return -LIZARDGPU_ERR_ARG;
    }
    lz_stream_finish_launch(d_frames, d_entries, (const u8*)d_blob, d_state, nFrames, fixedTotal, capacity, d_result, (u64*)d_offsets, stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_stream_seektable_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const LzStreamState* d_state, const uint64_t* d_offsets,
                                  uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, hipStream_t stream)
{
    if (!d_frames || !d_entries || !d_state || !d_offsets || nFrames == 0) {
        snprintf(t_err, sizeof t_err, "bad argument (null pointer or no frames)");
        return -LIZARDGPU_ERR_ARG;
    }
    lz_stream_seektable_launch(d_frames, d_entries, d_state, (const u64*)d_offsets, nFrames, fixedTotal, capacity, stream);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_unframes_walk_launch(const LzUnframesEntry* d_frames, uint32_t nFrames, int fill, uint64_t* d_offs, uint32_t* d_words,
                               struct LzWalkResult* d_res, hipStream_t stream)
{
    if (!d_frames || !d_res || nFrames == 0 || (fill && (!d_offs || !d_words))) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no frames)"); return -LIZARDGPU_ERR_ARG; }
    hipLaunchKernelGGL(lz_unframes_walk_kernel, dim3((nFrames + LZU_WALK_WAVES - 1u) / LZU_WALK_WAVES), dim3(64 * LZU_WALK_WAVES), 0, stream, d_frames, nFrames,
                       fill ? LZU_DECODE : LZU_WALK, fill ? (u64*)d_offs : nullptr, fill ? d_words : nullptr, d_res);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_unframes_decode_launch(LzCtx* c, const LzUnframesEntry* d_frames, const uint64_t* d_offs, const uint32_t* d_words, const uint32_t* d_recFrame,
                                 uint32_t* d_out, size_t nRecords, hipStream_t stream)
{
    return launch_unframes(*c, d_frames, (const u64*)d_offs, d_words, d_recFrame, d_out, nRecords, stream);
}
int   lzk_unframes_settle_launch(const LzUnframesEntry* d_frames, uint32_t nFrames, const uint32_t* d_out, LzUnframesResult* d_results,
                                 LzFramesEntry* d_hashTab, hipStream_t stream)
{
    if (!d_frames || !d_out || !d_results || !d_hashTab || nFrames == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no frames)"); return -LIZARDGPU_ERR_ARG; }
    hipLaunchKernelGGL(lz_unframes_settle_kernel, dim3((nFrames + LZU_WALK_WAVES - 1u) / LZU_WALK_WAVES), dim3(64 * LZU_WALK_WAVES), 0, stream, d_frames, nFrames,
                       d_out, d_results, d_hashTab);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_unframes_finish_launch(const LzUnframesEntry* d_frames, uint32_t nFrames, const LzFramesEntry* d_hashTab, LzUnframesResult* d_results,
                                 hipStream_t stream)
{
    if (!d_frames || !d_hashTab || !d_results || nFrames == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no frames)"); return -LIZARDGPU_ERR_ARG; }
    hipLaunchKernelGGL(lz_unframes_finish_kernel, dim3((nFrames + 255u) / 256u), dim3(256), 0, stream, d_frames, nFrames, d_hashTab, d_results);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_unstream_walk_launch(const void* d_src, size_t srcSize, LzStreamCtl* d_ctl, struct LzWalkResult* d_res, uint64_t* d_offs, uint32_t tableCap,
                               hipStream_t stream)
{
    if (!d_src || !d_ctl || !d_res || !d_offs || tableCap == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no table)"); return -LIZARDGPU_ERR_ARG; }
    hipLaunchKernelGGL(lz_unstream_walk_kernel, dim3(1), dim3(64), 0, stream, (const u8*)d_src, (u64)srcSize, d_ctl, d_res, (u64*)d_offs, tableCap);
    LZ_HIP(hipGetLastError());
    return 0;
}
// the grid of the plane kernels: a wave per tile up to eight waves per SIMD, a grid stride over the rest
static u32 planes_grid(const LzCtx* c, u32 nTiles)
{
    const u32 groups = (nTiles + LZP_WAVES - 1u) / LZP_WAVES, cap = (u32)c->cus * 8u;
    return groups < cap ? groups : cap;
}
int   lzk_planes_launch(LzCtx* c, const LzPlanesEntry* d_tab, uint32_t nEntries, uint32_t nTiles, int join, int bits, hipStream_t stream)
{
    static_assert(sizeof(LzPlanesEntry) == 32, "the table the host file fills");
    if (!d_tab || nEntries == 0 || nTiles == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no tiles)"); return -LIZARDGPU_ERR_ARG; }
    const dim3 grid(planes_grid(c, nTiles)), block(64 * LZP_WAVES);
    void (*const kernel)(const LzPlanesEntry*, u32, u32) = bits ? (join ? lz_bitplanes_join_kernel : lz_bitplanes_split_kernel)
                                                                : (join ? lz_planes_join_kernel : lz_planes_split_kernel);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, d_tab, nEntries, nTiles);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_planes_xor_launch(LzCtx* c, const LzPlanesXorEntry* d_tab, uint32_t nEntries, uint32_t nTiles, int join, int bits, hipStream_t stream)
{
    static_assert(sizeof(LzPlanesXorEntry) == 40, "the table the host file fills");
    if (!d_tab || nEntries == 0 || nTiles == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no tiles)"); return -LIZARDGPU_ERR_ARG; }
    const dim3 grid(planes_grid(c, nTiles)), block(64 * LZP_WAVES);
    void (*const kernel)(const LzPlanesXorEntry*, u32, u32) = bits ? (join ? lz_bitplanes_xor_join_kernel : lz_bitplanes_xor_split_kernel)
                                                                   : (join ? lz_planes_xor_join_kernel : lz_planes_xor_split_kernel);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, d_tab, nEntries, nTiles);
    LZ_HIP(hipGetLastError());
    return 0;
}
int   lzk_unslice_launch(LzCtx* c, const LzUnframesEntry* d_frames, const uint64_t* d_offs, const uint32_t* d_words, const LzSlicePick* d_picks,
                         void* d_dst, uint32_t* d_out, size_t nPicks, hipStream_t stream)
{
    static_assert(sizeof(LzSlicePick) == 24, "the table the host file fills");
    return launch_unslice(*c, d_frames, (const u64*)d_offs, d_words, d_picks, d_dst, d_out, nPicks, stream);
}
int   lzk_planes_range_launch(LzCtx* c, const LzPlanesRangeEntry* d_tab, uint32_t nEntries, const uint64_t* d_pieces, uint32_t nTiles, hipStream_t stream)
{
    static_assert(sizeof(LzPlanesRangeEntry) == 56, "the table the host file fills");
    if (!d_tab || !d_pieces || nEntries == 0 || nTiles == 0) { snprintf(t_err, sizeof t_err, "bad argument (null pointer or no tiles)"); return -LIZARDGPU_ERR_ARG; }
    const dim3 grid(planes_grid(c, nTiles)), block(64 * LZP_WAVES);
    hipLaunchKernelGGL(lz_planes_range_kernel, grid, block, 0, stream, d_tab, nEntries, (const u64*)d_pieces, nTiles);
    LZ_HIP(hipGetLastError());
    return 0;
}

#ifdef LZ_PROFILE
// Profile builds only: sum of the per-wave phase clocks since the last call (scratch slot tails), then reset.
int LizardGPU_profileDump(unsigned long long out[16])
{
    Guard g;
    for (int k = 0; k < 16; k++) out[k] = 0;
    if (g.rc) return g.rc;
    Ctx& c = *g.c;
    int rc = ctx_init(c);
    if (rc) return rc;
    (void)hipDeviceSynchronize();
    for (int w = 0; w < c.cus * LZ_MAX_WAVES; w++) {
        unsigned long long v[16];
        // the one-wave-per-block kernels keep a wave's record at the tail of its scratch slot; the producer / consumer kernels of
        // levels 10 / 30 (whose sequence buffers cover those tails) at the end of the workgroup's arena
        const size_t group = (size_t)(w / LZ_MAX_WAVES) * kScratchBytes;
        u8* const scratch = c.arena[0].scratch;
        u8* at = c.lastSplit ? scratch + group + kScratchBytes - (size_t)(w % LZ_MAX_WAVES + 1) * 128
                             : scratch + (size_t)(w + 1) * LZ_SCRATCH_BYTES - 128;
        if (hipMemcpy(v, at, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -LIZARDGPU_ERR_HIP;
        for (int k = 0; k < 15; k++) out[k] += v[k];
        (void)hipMemset(at, 0, sizeof v);
    }
    return 0;
}
#endif

int LizardGPU_arenasInUse(void)
{
    Guard g;
    if (g.rc) return 0;
    return g.c->ready ? g.c->nArenas : 0;
}

float LizardGPU_lastKernelMs(void)
{
    Guard g;
    if (g.rc) return -1.0f;
    Ctx& c = *g.c;
    if (c.hostKernelMs >= 0.0f) return c.hostKernelMs;
    float ms = -1.0f;
    if (c.lastEv1 && c.arena[0].timed && hipEventSynchronize(c.lastEv1) == hipSuccess) {
        if (hipEventElapsedTime(&ms, c.lastEv0, c.lastEv1) != hipSuccess) ms = -1.0f;
    }
    return ms;
}

}  // extern "C"
