/* tests/pipeline_fake.c — TEST INFRASTRUCTURE: the two host pipelines of the library — lizard_amd/csrc/lizard_pipeline_host.c
 * (run_host_job with its drain thread, stage_issue, stage_fetch; LizardGPU_decompressBlocks_host) and lizard_unframe_host.c
 * (LizardGPU_decompressFrame: three chunks in flight, staging reuse, packed / unpacked D2H, the hand-over to the host decoder, the
 * drain after an error) — compiled as units under test on a CPU, on the fake HIP runtime with DEFERRED streams of tests/fake_hip.c.
 * The lzk_* shims ENQUEUE closures: lz_unframe_record and the block decoder on the SIMT emulator (tests/pipeline_fake_emul.cpp), the
 * oracle as the compress kernels, a plain model of lz_scan_kernel + lz_gather_kernel.  lizard_frame_host.c, lizard_decode_host.c and
 * lizard_xxhash.c are linked as they are.  Every "kernel" checks that what it touches lies in live device memory.
 *   library : gcc -shared -Wl,-Bsymbolic ... (tests/test_pipeline_fake.py drives it through ctypes)
 * lizard_unframe_device.c (LizardGPU_decompressFrame_device / LizardGPU_frameIndex_device: walk, decode and checksum streams, two table
 * sets, the in-place pass and the staging pass, the device-side gather) is a third unit on the same fake: its walk is the real
 * lz_unframe_walk body on the emulator, its in-place launch a restatement of lz_unframe_inplace_kernel's slot rule.
 *   program : -DPIPELINE_FAKE_MAIN, for the sanitizer builds:  pipeline_fake core | threads [n] [rounds] | devcore | devthreads [n] [rounds]
 *             exit 0 = all good */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../lizard_amd/csrc/lizard_pipeline_host.c"      /* units under test, compiled into this harness */
#undef LZ_HIP
#include "../lizard_amd/csrc/lizard_unframe_host.c"
#undef LZ_HIP
#include "../lizard_amd/csrc/lizard_unframe_device.c"     /* (its statics are v_* / LZV_*, the host twin's uf_* / LZU_*) */
#include "device_fake_common.h"
#include "lizard_oracle.h"

unsigned emul_unframe_record(const void* payload, unsigned size, unsigned word, void* slot, unsigned cap, unsigned seed);
unsigned emul_decompress_block_raw(const void* src, unsigned n, void* dst, unsigned cap, unsigned seed);
void emul_walk_segment(const void* src, unsigned long long srcSize, unsigned long long startPos, unsigned long long budget,
                       unsigned long long tableCap, unsigned long long* offs, unsigned* words, void* res, unsigned seed);

/* ---- the shims of lizard_gpu_ctx.h ---- */
static LzCtx g_c;
static pthread_once_t g_ctxOnce = PTHREAD_ONCE_INIT;
static __thread char t_err[LZK_ERR_BYTES];
static int g_degraded;
/* pf_refuse_launch: the n-th launch of that kind from now answers -LIZARDGPU_ERR_HIP, once, and enqueues nothing */
enum { PF_WALK, PF_INPLACE, PF_UNFRAME, PF_KINDS };
static int g_refuse[PF_KINDS];
static int refused(int kind) { return g_refuse[kind] && !--g_refuse[kind]; }
static void ctx_once(void) { pthread_mutex_init(&g_c.mu, NULL); pthread_mutex_init(&g_c.comb.mu, NULL); pthread_cond_init(&g_c.comb.cv, NULL); }
void  lzk_guard_acquire(LzGuard* g) { pthread_once(&g_ctxOnce, ctx_once); pthread_mutex_lock(&g_c.mu); t_err[0] = 0; g->c = &g_c; g->saved = -1; g->rc = 0; }
/* the product drains what it left in flight before it gives the context back, also after an error or a give-up */
void  lzk_guard_release(LzGuard* g) { if (g->c) { fh_assert_idle("lzk_guard_release"); pthread_mutex_unlock(&g_c.mu); } g->c = NULL; }
char* lzk_err(void) { return t_err; }
int   lzk_ctx_init(LzCtx* c)
{
    int i;
    if (c->ready) return 0;
    for (i = 0; i < LZ_STAGES; i++) {
        LzStage* s = &c->stage[i];
        hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
        hipEventCreate(&s->k0); hipEventCreate(&s->k1); hipEventCreate(&s->meta); hipEventCreate(&s->done); hipEventCreate(&s->up);
    }
    c->ready = 1;
    return 0;
}
int   lzk_clamp_level(int level) { return level > 49 ? 49 : level < 10 ? 17 : level; }
LzCtx* lzk_ctx_peek(void) { pthread_once(&g_ctxOnce, ctx_once); return &g_c; }
int   lzk_dev_alloc(LzCtx* c, void** p, size_t n) { c->devBytes += n; return hipMalloc(p, n) == hipSuccess ? 0 : -LIZARDGPU_ERR_NOMEM; }
void  lzk_dev_free(LzCtx* c, void* p, size_t n) { c->devBytes -= n; (void)hipFree(p); }
size_t lzk_budget(void) { return 0; }
size_t lzk_budget_room_for_staging(const LzCtx* c) { (void)c; return (size_t)-1; }
int LizardGPU_levelSupported(int level) { return lzo_level_supported(lzk_clamp_level(level)); }
const char* LizardGPU_lastError(void) { return t_err; }
void lzgpu_note_degraded(const char* what, int level) { (void)what; (void)level; __atomic_add_fetch(&g_degraded, 1, __ATOMIC_RELAXED); }

/* lz_unframe_kernel: one wave per record, in whatever order the waves claim them */
typedef struct { const uint8_t* src; const uint64_t* offs; const uint32_t* words; size_t n; uint8_t* slots; size_t slotBytes; uint32_t *outSizes, *packSizes; } UnframeK;
static void unframe_kernel(void* a)
{
    const UnframeK* k = (const UnframeK*)a;
    const uint32_t cap = k->slotBytes > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)k->slotBytes;
    uint32_t* order = (uint32_t*)malloc(k->n * sizeof *order);
    size_t i;
    if (!fh_check_dev(k->offs, 8 * k->n, "unframe: payload offsets") || !fh_check_dev(k->words, 4 * k->n, "unframe: words")
        || !fh_check_dev(k->outSizes, 4 * k->n, "unframe: outSizes") || !fh_check_dev(k->packSizes, 4 * k->n, "unframe: packSizes")
        || !fh_check_dev(k->slots, k->n * k->slotBytes, "unframe: slots")) { free(order); return; }
    dfc_shuffled(order, k->n);
    for (i = 0; i < k->n; i++) {
        const uint32_t b = order[i], word = k->words[b], size = word & 0x7FFFFFFFu;
        uint32_t r;
        if (size && size <= cap && !fh_check_dev(k->src + k->offs[b], size, "unframe: a record's payload")) continue;
        r = emul_unframe_record(k->src + k->offs[b], size, word, k->slots + (size_t)b * k->slotBytes, cap, fh_rand() | 1u);
        k->outSizes[b] = r; k->packSizes[b] = r >= 0xFFFFFFFEu ? 0u : r;
    }
    free(order);
}
int lzk_launch_unframe(LzCtx* c, const void* d_src, const uint64_t* d_payloadOffsets, const uint32_t* d_words, size_t nRecords, void* d_slots,
                       size_t slotBytes, uint32_t* d_outSizes, uint32_t* d_packSizes, hipStream_t stream)
{
    UnframeK k;
    if (!d_src || !d_payloadOffsets || !d_words || !d_slots || !d_outSizes || !d_packSizes || nRecords == 0 || slotBytes == 0) return -LIZARDGPU_ERR_ARG;
    if (refused(PF_UNFRAME)) { snprintf(t_err, sizeof t_err, "lzk_launch_unframe: refused by the test"); return -LIZARDGPU_ERR_HIP; }
    k.src = (const uint8_t*)d_src; k.offs = d_payloadOffsets; k.words = d_words; k.n = nRecords; k.slots = (uint8_t*)d_slots; k.slotBytes = slotBytes;
    k.outSizes = d_outSizes; k.packSizes = d_packSizes;
    c->hostKernelMs = -1.0f;
    return fh_enqueue_kernel(stream, unframe_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* lz_unframe_inplace_kernel: the slots are places inside the caller's buffer, the last one as short as the room that is left */
typedef struct { const uint8_t* src; const uint64_t* offs; const uint32_t* words; size_t n; uint8_t* dst; size_t slotBytes, dstRoom; uint32_t *outSizes, *packSizes; } InplaceK;
static void inplace_kernel(void* a)
{
    const InplaceK* k = (const InplaceK*)a;
    uint32_t* order = (uint32_t*)malloc(k->n * sizeof *order);
    size_t i;
    if (!fh_check_dev(k->offs, 8 * k->n, "inplace: payload offsets") || !fh_check_dev(k->words, 4 * k->n, "inplace: words")
        || !fh_check_dev(k->outSizes, 4 * k->n, "inplace: outSizes") || !fh_check_dev(k->packSizes, 4 * k->n, "inplace: packSizes")
        || !fh_check_dev(k->dst, k->dstRoom, "inplace: dst[0..dstRoom)")) { free(order); return; }
    dfc_shuffled(order, k->n);
    for (i = 0; i < k->n; i++) {
        const uint32_t b = order[i], word = k->words[b], size = word & 0x7FFFFFFFu;
        const size_t at = (size_t)b * k->slotBytes;
        uint32_t r = 0xFFFFFFFFu;
        if (at < k->dstRoom) {
            size_t room = k->dstRoom - at;
            if (room > k->slotBytes) room = k->slotBytes;
            if (room > 0x7FFFFFFFull) room = 0x7FFFFFFFull;
            if (size && size <= room && !fh_check_dev(k->src + k->offs[b], size, "inplace: a record's payload")) continue;
            r = emul_unframe_record(k->src + k->offs[b], size, word, k->dst + at, (uint32_t)room, fh_rand() | 1u);
        }
        k->outSizes[b] = r; k->packSizes[b] = r >= 0xFFFFFFFEu ? 0u : r;
    }
    free(order);
}
int lzk_launch_unframe_inplace(LzCtx* c, const void* d_src, const uint64_t* d_payloadOffsets, const uint32_t* d_words, size_t nRecords,
                               void* d_dst, size_t slotBytes, size_t dstRoom, uint32_t* d_outSizes, uint32_t* d_packSizes, hipStream_t stream)
{
    InplaceK k;
    if (!d_src || !d_payloadOffsets || !d_words || !d_dst || !d_outSizes || !d_packSizes || nRecords == 0 || nRecords > 0xFFFFFFFFu || slotBytes == 0
        || dstRoom == 0 || (nRecords - 1) > (dstRoom - 1) / slotBytes) { snprintf(t_err, sizeof t_err, "lzk_launch_unframe_inplace: bad argument"); return -LIZARDGPU_ERR_ARG; }
    if (refused(PF_INPLACE)) { snprintf(t_err, sizeof t_err, "lzk_launch_unframe_inplace: refused by the test"); return -LIZARDGPU_ERR_HIP; }
    k.src = (const uint8_t*)d_src; k.offs = d_payloadOffsets; k.words = d_words; k.n = nRecords; k.dst = (uint8_t*)d_dst; k.slotBytes = slotBytes;
    k.dstRoom = dstRoom; k.outSizes = d_outSizes; k.packSizes = d_packSizes;
    c->hostKernelMs = -1.0f;
    return fh_enqueue_kernel(stream, inplace_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* lz_unframe_walk_kernel: the real walk on the emulator, one wave */
typedef struct { const uint8_t* src; size_t srcSize, startPos, budget, tableCap; uint64_t* offs; uint32_t* words; LzWalkResult* res; } WalkK;
static void walk_kernel(void* a)
{
    const WalkK* k = (const WalkK*)a;
    if ((k->srcSize && !fh_check_dev(k->src, k->srcSize, "walk: src[0..srcSize)")) || !fh_check_dev(k->res, sizeof *k->res, "walk: result record")
        || (k->offs && k->tableCap && !fh_check_dev(k->offs, 8 * k->tableCap, "walk: offset table"))
        || (k->words && k->tableCap && !fh_check_dev(k->words, 4 * k->tableCap, "walk: word table"))) return;
    emul_walk_segment(k->src, k->srcSize, k->startPos, k->budget, k->tableCap, (unsigned long long*)k->offs, k->words, k->res, fh_rand() | 1u);
}
int lzk_launch_walk(LzCtx* c, const void* d_src, size_t srcSize, size_t startPos, size_t budget, size_t tableCap, uint64_t* d_offs,
                    uint32_t* d_words, struct LzWalkResult* d_res, hipStream_t stream)
{
    WalkK k;
    (void)c;
    if ((!d_src && srcSize) || !d_res || startPos > srcSize) { snprintf(t_err, sizeof t_err, "lzk_launch_walk: bad argument"); return -LIZARDGPU_ERR_ARG; }
    if (refused(PF_WALK)) { snprintf(t_err, sizeof t_err, "lzk_launch_walk: refused by the test"); return -LIZARDGPU_ERR_HIP; }
    k.src = (const uint8_t*)d_src; k.srcSize = srcSize; k.startPos = startPos; k.budget = budget; k.tableCap = tableCap; k.offs = d_offs; k.words = d_words;
    k.res = d_res;
    return fh_enqueue_kernel(stream, walk_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* lz_decompress_kernel */
typedef struct { const uint8_t* src; const uint64_t* offs; size_t srcStride; const uint32_t* srcSizes; size_t n; uint8_t* dst; size_t dstStride; uint32_t* outSizes; } DecK;
static void decompress_kernel(void* a)
{
    const DecK* k = (const DecK*)a;
    const uint32_t cap = k->dstStride > 0x7E000000ull ? 0x7E000000u : (uint32_t)k->dstStride;
    uint32_t* order = (uint32_t*)malloc(k->n * sizeof *order);
    size_t i;
    if ((k->offs && !fh_check_dev(k->offs, 8 * (k->n + 1), "decompress: offsets")) || (!k->offs && !fh_check_dev(k->srcSizes, 4 * k->n, "decompress: sizes"))
        || !fh_check_dev(k->outSizes, 4 * k->n, "decompress: outSizes") || !fh_check_dev(k->dst, k->n * k->dstStride, "decompress: slots")) { free(order); return; }
    dfc_shuffled(order, k->n);
    for (i = 0; i < k->n; i++) {
        const uint32_t b = order[i];
        const uint8_t* in = k->offs ? k->src + k->offs[b] : k->src + (size_t)b * k->srcStride;
        const uint32_t n = k->offs ? (uint32_t)(k->offs[b + 1] - k->offs[b]) : k->srcSizes[b];
        if (n && !fh_check_dev(in, n, "decompress: a block's input")) continue;
        k->outSizes[b] = emul_decompress_block_raw(in, n, k->dst + (size_t)b * k->dstStride, cap, fh_rand() | 1u);
    }
    free(order);
}
int lzk_launch_decompress(LzCtx* c, const void* d_src, const uint64_t* d_offsets, size_t srcStride, const uint32_t* d_srcSizes, size_t nBlocks,
                          void* d_dst, size_t dstStride, uint32_t* d_outSizes, hipStream_t stream)
{
    DecK k;
    if (!d_src || !d_dst || !d_outSizes || (!d_offsets && !d_srcSizes) || nBlocks == 0 || dstStride == 0) return -LIZARDGPU_ERR_ARG;
    k.src = (const uint8_t*)d_src; k.offs = d_offsets; k.srcStride = srcStride; k.srcSizes = d_srcSizes; k.n = nBlocks; k.dst = (uint8_t*)d_dst;
    k.dstStride = dstStride; k.outSizes = d_outSizes;
    c->hostKernelMs = -1.0f;
    return fh_enqueue_kernel(stream, decompress_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

/* the block kernels: the oracle, block by block */
typedef struct { const uint8_t* src; size_t nb, blockSize, last; uint8_t* dst; size_t stride; uint32_t* sizes; int level; const uint32_t* srcSizes; const uint64_t* srcOffsets; } CompK;
static void compress_kernel(void* a)
{
    const CompK* k = (const CompK*)a;
    uint32_t* order = (uint32_t*)malloc(k->nb * sizeof *order);
    size_t i;
    if (!fh_check_dev(k->sizes, 4 * k->nb, "compress: sizes") || !fh_check_dev(k->dst, k->nb * k->stride, "compress: slots")
        || (k->srcSizes && (!fh_check_dev(k->srcSizes, 4 * k->nb, "compress: srcSizes") || !fh_check_dev(k->srcOffsets, 8 * k->nb, "compress: srcOffsets")))) { free(order); return; }
    dfc_shuffled(order, k->nb);
    for (i = 0; i < k->nb; i++) {
        const size_t b = order[i];
        const size_t n = k->srcSizes ? k->srcSizes[b] : (b + 1 == k->nb ? k->last : k->blockSize);
        const uint8_t* in = k->src + (k->srcOffsets ? k->srcOffsets[b] : b * k->blockSize);
        if (!fh_check_dev(in, n, "compress: a block's input")) continue;
        k->sizes[b] = (uint32_t)lzo_compress(in, k->dst + b * k->stride, (int)n, (int)k->stride, k->level);
    }
    free(order);
}
int lzk_launch(LzCtx* c, const void* d_src, size_t nBlocks, size_t blockSize, size_t lastBlockSize, void* d_dst, size_t dstStride,
               uint32_t* d_sizes, int level, hipStream_t stream, hipEvent_t k0, hipEvent_t k1, const uint32_t* d_srcSizes, const uint64_t* d_srcOffsets)
{
    CompK k;
    (void)c;
    k.src = (const uint8_t*)d_src; k.nb = nBlocks; k.blockSize = blockSize; k.last = lastBlockSize; k.dst = (uint8_t*)d_dst; k.stride = dstStride;
    k.sizes = d_sizes; k.level = lzk_clamp_level(level); k.srcSizes = d_srcSizes; k.srcOffsets = d_srcOffsets;
    if (k0) hipEventRecord(k0, stream);
    if (fh_enqueue_kernel(stream, compress_kernel, &k, sizeof k) != hipSuccess) return -LIZARDGPU_ERR_HIP;
    if (k1) hipEventRecord(k1, stream);
    return 0;
}

/* lz_scan_kernel + lz_gather_kernel (lz_pack.h), plainly */
typedef struct { const uint8_t *in, *slots; size_t slot; const uint32_t* sizes; uint64_t* offsets; uint8_t* packed; uint32_t nb, blockSize, last; int mode; } PackK;
static void pack_kernel(void* a)
{
    const PackK* k = (const PackK*)a;
    uint64_t run = 0;
    uint32_t b;
    if (!fh_check_dev(k->sizes, 4 * (size_t)k->nb, "pack: sizes") || !fh_check_dev(k->offsets, 8 * ((size_t)k->nb + 1), "pack: offsets")) return;
    for (b = 0; b < k->nb; b++) {
        const uint32_t n = b == k->nb - 1u ? k->last : k->blockSize, cs = k->sizes[b];
        const int raw = k->mode == LZK_PACK_FRAME && n != 1u && (cs == 0u || cs > n - 1u);
        k->offsets[b] = run;
        run += k->mode == LZK_PACK_PAYLOAD ? cs : 4u + (raw ? n : cs);
    }
    k->offsets[k->nb] = run;
    if (run && !fh_check_dev(k->packed, run, "pack: packed output")) return;
    for (b = 0; b < k->nb; b++) {
        const uint32_t n = b == k->nb - 1u ? k->last : k->blockSize, cs = k->sizes[b];
        uint8_t* out = k->packed + k->offsets[b];
        const uint8_t* from = k->slots + (size_t)b * k->slot;
        uint32_t len = cs;
        if (k->mode == LZK_PACK_FRAME) {
            const int raw = n != 1u && (cs == 0u || cs > n - 1u);
            const uint32_t word = raw ? (n | 0x80000000u) : cs;
            out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
            out += 4;
            if (raw) { from = k->in + (size_t)b * k->blockSize; len = n; }
        }
        if (len && fh_check_dev(from, len, "pack: a record's source")) memcpy(out, from, len);
    }
}
void lzk_pack_launch(const void* d_in, const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, void* d_packed,
                     uint32_t nb, uint32_t blockSize, uint32_t lastBlockSize, int mode, hipStream_t stream)
{
    PackK k;
    k.in = (const uint8_t*)d_in; k.slots = (const uint8_t*)d_slots; k.slot = slot; k.sizes = d_sizes; k.offsets = d_offsets; k.packed = (uint8_t*)d_packed;
    k.nb = nb; k.blockSize = blockSize; k.last = lastBlockSize; k.mode = mode;
    (void)fh_enqueue_kernel(stream, pack_kernel, &k, sizeof k);
}

/* ---- controls for the tests ---- */
void pf_set_chunk_bytes(size_t n) { LzGuard g; lzk_guard_acquire(&g); g_chunk_bytes = n; lzk_guard_release(&g); }
void pf_refuse_launch(int kind, int nth) { LzGuard g; lzk_guard_acquire(&g); if (kind >= 0 && kind < PF_KINDS) g_refuse[kind] = nth; lzk_guard_release(&g); }
int  pf_degraded(void) { return __atomic_load_n(&g_degraded, __ATOMIC_RELAXED); }
/* what LizardGPU_shutdown does to the stages: the next call allocates (poisoned) buffers afresh */
void pf_shutdown(void)
{
    LzGuard g;
    int i;
    lzk_guard_acquire(&g);
    (void)hipDeviceSynchronize();
    for (i = 0; i < LZ_STAGES && g_c.ready; i++) {
        LzStage* s = &g_c.stage[i];
        if (s->h_in) (void)hipHostFree(s->h_in);
        if (s->h_out) (void)hipHostFree(s->h_out);
        if (s->h_aux) (void)hipHostFree(s->h_aux);
        if (s->d_in) (void)hipFree(s->d_in);
        if (s->d_slots) (void)hipFree(s->d_slots);
        if (s->d_packed) (void)hipFree(s->d_packed);
        if (s->d_aux) (void)hipFree(s->d_aux);
        free_meta(s);
        (void)hipEventDestroy(s->k0); (void)hipEventDestroy(s->k1); (void)hipEventDestroy(s->meta); (void)hipEventDestroy(s->done); (void)hipEventDestroy(s->up);
        (void)hipStreamDestroy(s->stream);
        memset(s, 0, sizeof *s);
    }
    if (g_c.dfTab) { (void)hipFree(g_c.dfTab); g_c.dfTab = NULL; g_c.dfTabCap = 0; }
    g_c.ready = 0; g_c.devBytes = 0;
    lzk_guard_release(&g);
}

#ifdef PIPELINE_FAKE_MAIN
/* ---- the program form: core cases and the thread test, for the sanitizer builds ---- */
#define CHECK(cond, ...) DFC_CHECK("pipeline_fake", cond, __VA_ARGS__)
typedef struct { uint8_t* frame; size_t bytes; const uint8_t* plain; size_t n; } Frame;
static uint8_t *g_data, *g_noise;
static size_t g_n, g_noiseN;
static Frame g_frames[4]; static int g_nFrames;

static Frame make_frame(const uint8_t* data, size_t n, int level, int bsid, int mode, int flushAt)
{
    LizardF_preferences_t p;
    Frame f;
    size_t cap, r;
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)bsid; p.frameInfo.blockMode = (LizardF_blockMode_t)mode; p.frameInfo.contentChecksumFlag = (LizardF_contentChecksum_t)1;
    p.compressionLevel = level;
    cap = LizardF_compressFrameBound(n, &p) + ((size_t)1 << 20);
    f.frame = (uint8_t*)malloc(cap); f.plain = data; f.n = n; f.bytes = 0;
    if (!flushAt) r = LizardF_compressFrame(f.frame, cap, data, n, &p);
    else {                                                  /* a flush in the middle of a block: a short record inside the frame */
        LizardF_compressionContext_t cc;
        size_t pos;
        LizardF_createCompressionContext(&cc, LIZARDF_VERSION);
        pos = LizardF_compressBegin(cc, f.frame, cap, &p);
        pos += LizardF_compressUpdate(cc, f.frame + pos, cap - pos, data, (size_t)flushAt, NULL);
        pos += LizardF_flush(cc, f.frame + pos, cap - pos, NULL);
        pos += LizardF_compressUpdate(cc, f.frame + pos, cap - pos, data + flushAt, n - (size_t)flushAt, NULL);
        pos += LizardF_compressEnd(cc, f.frame + pos, cap - pos, NULL);
        LizardF_freeCompressionContext(cc);
        r = pos;
    }
    if (LizardF_isError(r) || r > cap) { fprintf(stderr, "pipeline_fake: could not build a frame\n"); exit(2); }
    f.bytes = r;
    return f;
}
static int decode_check(const Frame* f, int pinned, uint8_t* out /* f->n + 64 */)
{
    uint8_t* src = (uint8_t*)malloc(f->bytes + 16);
    size_t used = 1, r;
    memcpy(src + 3, f->frame, f->bytes);                  /* an odd offset; exact-size: a read behind the frame is a sanitizer report */
    if (pinned) fh_register_pinned(src, f->bytes + 16);
    memset(out, 0xC3, f->n + 64);
    r = LizardGPU_decompressFrame(out, f->n, src + 3, f->bytes, &used);
    CHECK(r == f->n && used == f->bytes, "decompressFrame returned %zu (consumed %zu) for %zu bytes: %s", r, used, f->n, LizardGPU_lastError());
    CHECK(!memcmp(out, f->plain, f->n) && out[f->n] == 0xC3, "decoded bytes differ");
    r = LizardGPU_decompressFrame(out, f->n - 1, src + 3, f->bytes, &used);
    CHECK(r == LZ_FRAME_E(dstMaxSize_tooSmall) && used == 0, "capacity n - 1: %zu", r);
    if (pinned) fh_unregister_pinned(src);
    free(src);
    return 0;
}
static int compress_check(const uint8_t* data, size_t n, size_t bs, int level, uint8_t* scratch)
{
    const size_t nb = (n + bs - 1) / bs, last = n - (nb - 1) * bs, stride = (size_t)lzo_compress_bound((int)bs);
    uint8_t* dst = (uint8_t*)malloc(nb * stride);
    uint8_t* back = (uint8_t*)malloc(nb * bs);
    uint32_t* sizes = (uint32_t*)malloc(nb * 4);
    uint32_t* outSizes = (uint32_t*)malloc(nb * 4);
    uint64_t* offs = (uint64_t*)malloc((nb + 1) * 8);
    size_t b;
    int rc;
    rc = LizardGPU_compressBlocks_host_packed(data, nb, bs, last, dst, nb * stride, offs, sizes, level);
    CHECK(rc == 0, "compressBlocks_host_packed: %d %s", rc, LizardGPU_lastError());
    for (b = 0; b < nb; b++) {
        const int want = lzo_compress(data + b * bs, scratch, (int)(b + 1 == nb ? last : bs), (int)stride, level);
        CHECK((int)sizes[b] == want && offs[b + 1] - offs[b] == sizes[b] && !memcmp(dst + offs[b], scratch, sizes[b]), "block %zu differs from the oracle", b);
    }
    fh_allow_pageable(1);                                  /* this entry hands caller memory to the async copies and synchronises before it returns */
    rc = LizardGPU_decompressBlocks_host(dst, offs, nb, back, bs, outSizes);
    fh_allow_pageable(0);
    CHECK(rc == 0, "decompressBlocks_host: %d", rc);
    for (b = 0; b < nb; b++) CHECK(outSizes[b] == (b + 1 == nb ? last : bs) && !memcmp(back + b * bs, data + b * bs, outSizes[b]), "block %zu does not round-trip", b);
    rc = LizardGPU_compressBlocks_host_packed(data, nb, bs, last, dst, (size_t)offs[nb] - 1, offs, sizes, level);
    CHECK(rc == -LIZARDGPU_ERR_ARG, "a packed capacity one byte short: %d", rc);
    rc = LizardGPU_compressBlocks_host(data, nb, bs, last, dst, stride, sizes, level);
    CHECK(rc == 0 && (int)sizes[0] == lzo_compress(data, scratch, (int)(nb == 1 ? last : bs), (int)stride, level) && !memcmp(dst, scratch, sizes[0]), "compressBlocks_host after an error");
    free(dst); free(back); free(sizes); free(outSizes); free(offs);
    return 0;
}
static void setup(size_t n)
{
    g_n = n; g_data = (uint8_t*)malloc(n); lzo_datagen(g_data, n, 0.5, 0.0, 77u);
    fh_set_schedule(FH_EAGER, 1);
    pf_set_chunk_bytes((size_t)256 << 10);
    g_frames[g_nFrames++] = make_frame(g_data, n, 10, 1, 1, 0);
    g_frames[g_nFrames++] = make_frame(g_data, n, 10, 1, 0, 0);
    g_frames[g_nFrames++] = make_frame(g_data, n, 10, 1, 1, 200001);
}
static int core(void)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 }, { FH_RANDOM, 12 }, { FH_RANDOM, 13 } };
    uint8_t* out;
    size_t s, c;
    int f;
    setup(5 * 131072 + 4321);
    out = (uint8_t*)malloc(g_n + (size_t)lzo_compress_bound(1 << 17) + 64);
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++)
        for (c = 0; c < 2; c++) {
            fh_set_schedule(sched[s].mode, sched[s].seed);
            pf_set_chunk_bytes(c ? (size_t)1 << 20 : (size_t)256 << 10);
            if (s == 1) pf_shutdown();
            for (f = 0; f < g_nFrames; f++) {
                if (decode_check(&g_frames[f], (f + (int)c) & 1, out)) { fprintf(stderr, "  (frame %d, schedule %d seed %u, chunk %zu)\n", f, sched[s].mode, sched[s].seed, c); return 1; }
            }
            {   /* a damaged record in a middle chunk, then a good call */
                Frame bad = g_frames[0];
                size_t used;
                bad.frame = (uint8_t*)malloc(bad.bytes); memcpy(bad.frame, g_frames[0].frame, bad.bytes);
                memset(bad.frame + bad.bytes / 2, 0xFF, 40);
                fh_register_pinned(bad.frame, bad.bytes);
                CHECK(LizardF_isError(LizardGPU_decompressFrame(out, g_n, bad.frame, bad.bytes, &used)), "a damaged frame was accepted");
                fh_unregister_pinned(bad.frame);
                free(bad.frame);
                if (decode_check(&g_frames[0], 0, out)) return 1;
            }
            if (compress_check(g_data, c ? g_n : g_n / 2, 131072, s & 1 ? 30 : 10, out)) { fprintf(stderr, "  (schedule %d seed %u)\n", sched[s].mode, sched[s].seed); return 1; }
        }
    printf("pipeline_fake core: ok, %llu ops\n", fh_ops_run());
    return 0;
}

typedef struct { int id, rounds, bad; } Worker;
static void* worker(void* a)
{
    Worker* w = (Worker*)a;
    uint8_t* out = (uint8_t*)malloc(g_n + (size_t)lzo_compress_bound(1 << 17) + 64);
    unsigned r = 977u * (unsigned)(w->id + 1);
    int i;
    for (i = 0; i < w->rounds && !w->bad; i++) {
        r = r * 1664525u + 1013904223u;
        if (w->id == 0 && i == 0 && g_noise) {              /* chunks above 16 MiB: the copy threads of par_memcpy, on both sides */
            const size_t bs = (size_t)1 << 20, nb = g_noiseN / bs, cap = nb * (size_t)lzo_compress_bound((int)bs);
            uint8_t* dst = (uint8_t*)malloc(cap);
            uint64_t* offs = (uint64_t*)malloc((nb + 1) * 8);
            size_t b;
            pf_set_chunk_bytes((size_t)17 << 20);             /* (read under the context lock; the others see it for a call or two) */
            w->bad |= LizardGPU_compressBlocks_host_packed(g_noise, nb, bs, bs, dst, cap, offs, NULL, 10) != 0;
            pf_set_chunk_bytes((size_t)256 << 10);
            for (b = 0; b < nb && !w->bad; b++) w->bad |= (int)(offs[b + 1] - offs[b]) != lzo_compress(g_noise + b * bs, out, (int)bs, lzo_compress_bound((int)bs), 10);
            free(dst); free(offs);
        } else if ((r >> 8) % 3u) w->bad |= decode_check(&g_frames[(r >> 12) % (unsigned)g_nFrames], (int)((r >> 16) & 1u), out);
        else w->bad |= compress_check(g_data, g_n, 131072, (r >> 20) & 1u ? 10 : 21, out);
    }
    free(out);
    return NULL;
}
static void* watchdog(void* a) { (void)a; sleep(900); fprintf(stderr, "pipeline_fake: HANG (watchdog)\n"); _exit(3); return NULL; }
static int threads(int n, int rounds, int big)
{
    pthread_t th[64], wd;
    Worker w[64];
    int i, bad = 0;
    if (n > 64) return 2;
    setup(5 * 131072 + 99);
    if (big) { g_noiseN = (size_t)34 << 20; g_noise = (uint8_t*)malloc(g_noiseN); lzo_datagen(g_noise, g_noiseN, 0.0, 1.0, 5u); }
    pf_set_chunk_bytes((size_t)256 << 10);
    fh_set_schedule(FH_RANDOM, 4242);
    pthread_create(&wd, NULL, watchdog, NULL); pthread_detach(wd);
    for (i = 0; i < n; i++) { w[i].id = i; w[i].rounds = rounds; w[i].bad = 0; pthread_create(&th[i], NULL, worker, &w[i]); }
    for (i = 0; i < n; i++) { pthread_join(th[i], NULL); bad += w[i].bad; }
    printf("pipeline_fake threads: %d threads x %d rounds, %d bad, %llu ops\n", n, rounds, bad, fh_ops_run());
    return bad ? 1 : 0;
}

/* ---- LizardGPU_decompressFrame_device: fake device buffers with canary margins, uploaded on a caller's stream that is not waited for ---- */
#define DV_G 4096
static hipStream_t g_user;
static pthread_mutex_t g_userMu = PTHREAD_MUTEX_INITIALIZER;      /* one caller's stream for all threads: the enqueues of a call stay together */
static int g_syncUpload;        /* the thread test: another thread may release the context meanwhile, and that asserts that ALL queues are empty */
static int dev_decode(const Frame* f, size_t cap, unsigned flags, size_t wantResult, int compare)
{
    uint8_t *dsrc = NULL, *ddst = NULL, *hsrc = NULL, *hdst = NULL;
    const size_t sn = f->bytes + 2 * DV_G, dn = cap + 2 * DV_G;
    size_t used = 1, r, i;
    int bad = 0;
    CHECK(hipMalloc((void**)&dsrc, sn) == hipSuccess && hipMalloc((void**)&ddst, dn) == hipSuccess
          && hipHostMalloc((void**)&hsrc, sn, 0) == hipSuccess && hipHostMalloc((void**)&hdst, dn, 0) == hipSuccess, "allocation");
    memset(hsrc, 0x5A, sn); memcpy(hsrc + DV_G, f->frame, f->bytes); memset(hdst, 0xC3, dn);
    pthread_mutex_lock(&g_userMu);
    if (!g_user) hipStreamCreateWithFlags(&g_user, hipStreamNonBlocking);
    if (g_syncUpload) { hipMemcpy(dsrc, hsrc, sn, hipMemcpyHostToDevice); hipMemcpy(ddst, hdst, dn, hipMemcpyHostToDevice); }
    else { hipMemcpyAsync(dsrc, hsrc, sn, hipMemcpyHostToDevice, g_user); hipMemcpyAsync(ddst, hdst, dn, hipMemcpyHostToDevice, g_user); }
    r = LizardGPU_decompressFrame_device(ddst + DV_G, cap, dsrc + DV_G, f->bytes, &used, flags, g_user);
    pthread_mutex_unlock(&g_userMu);
    memset(hdst, 0, dn);
    hipMemcpy(hdst, ddst, dn, hipMemcpyDeviceToHost);
    for (i = 0; i < DV_G; i++) bad |= hdst[i] != 0xC3 || hdst[DV_G + cap + i] != 0xC3;
    if (!bad && (compare == 2 ? !LizardF_isError(r) : r != wantResult)) bad = 2;    /* compare 2: any refusal */
    if (!bad && !LizardF_isError(r) && (used != f->bytes || (compare == 1 && memcmp(hdst + DV_G, f->plain, r)))) bad = 3;
    if (!bad && LizardF_isError(r) && used != 0) bad = 4;
    hipFree(dsrc); hipFree(ddst); hipHostFree(hsrc); hipHostFree(hdst);
    CHECK(!bad, "decompressFrame_device: %s (result %zu, wanted %zu, consumed %zu of %zu, capacity %zu): %s",
          bad == 1 ? "a canary margin of d_dst changed" : bad == 2 ? "unexpected result" : bad == 3 ? "wrong bytes or consumed count" : "consumed set on an error",
          r, wantResult, used, f->bytes, cap, LizardGPU_lastError());
    return 0;
}
static int dev_check(const Frame* f)
{
    if (dev_decode(f, f->n, 0, f->n, 1)) return 1;
    if (dev_decode(f, f->n + 77, 1u, f->n, 1)) return 1;
    return dev_decode(f, f->n - 1, 0, LZ_FRAME_E(dstMaxSize_tooSmall), 0);
}
static int devcore(void)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 }, { FH_RANDOM, 12 }, { FH_RANDOM, 13 } };
    static const char* const budget[] = { NULL, "1", "2", "3", "1" };
    uint8_t* out;
    size_t s;
    int f;
    setup(4 * 131072 + 4321);
    out = (uint8_t*)malloc(g_n + 64);
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++) {
        Frame bad = g_frames[0], cut = g_frames[0];
        fh_set_schedule(sched[s].mode, sched[s].seed);
        pf_set_chunk_bytes(s & 1 ? (size_t)1 << 20 : (size_t)256 << 10);
        if (budget[s]) setenv("LIZARDGPU_WALK_RECORDS", budget[s], 1); else unsetenv("LIZARDGPU_WALK_RECORDS");
        if (s == 1) pf_shutdown();
        for (f = 0; f < g_nFrames; f++)
            if (dev_check(&g_frames[f])) { fprintf(stderr, "  (frame %d, schedule %d seed %u)\n", f, sched[s].mode, sched[s].seed); return 1; }
        /* capacity edges: a slot border with records to come, inside a slot, nothing */
        if (dev_decode(&g_frames[0], 2 * 131072, 0, LZ_FRAME_E(dstMaxSize_tooSmall), 0) || dev_decode(&g_frames[0], 3 * 131072 + 100, 0, LZ_FRAME_E(dstMaxSize_tooSmall), 0)
            || dev_decode(&g_frames[0], 0, 0, LZ_FRAME_E(dstMaxSize_tooSmall), 0)) return 1;
        /* a damaged record, a frame cut inside its checksum, a stored checksum that is wrong (and skipped), a launch that is refused */
        bad.frame = (uint8_t*)malloc(bad.bytes); memcpy(bad.frame, g_frames[0].frame, bad.bytes);
        memset(bad.frame + bad.bytes / 2, 0xFF, 40);
        if (dev_decode(&bad, g_n, 0, 0, 2)) return 1;
        memcpy(bad.frame, g_frames[0].frame, bad.bytes); bad.frame[bad.bytes - 1] ^= 1;
        if (dev_decode(&bad, g_n, 0, LZ_FRAME_E(contentChecksum_invalid), 0) || dev_decode(&bad, g_n, 1u, g_n, 1)) return 1;
        free(bad.frame);
        cut.bytes -= 2;
        if (dev_decode(&cut, g_n, 0, LZ_FRAME_E(GENERIC), 0)) return 1;
        pf_refuse_launch((int)(s & 1), s ? 2 : 1);           /* the walk or the in-place launch, of the first or the second segment */
        if (dev_decode(&g_frames[2], g_n, 0, LZ_FRAME_E(GENERIC), 0)) return 1;
        if (dev_check(&g_frames[2]) || decode_check(&g_frames[1], (int)(s & 1), out)) return 1;
    }
    unsetenv("LIZARDGPU_WALK_RECORDS");
    free(out);
    printf("pipeline_fake devcore: ok, %llu ops\n", fh_ops_run());
    return 0;
}
static void* dev_worker(void* a)
{
    Worker* w = (Worker*)a;
    uint8_t* out = (uint8_t*)malloc(g_n + (size_t)lzo_compress_bound(1 << 17) + 64);
    unsigned r = 977u * (unsigned)(w->id + 1);
    int i;
    for (i = 0; i < w->rounds && !w->bad; i++) {
        const Frame* f;
        r = r * 1664525u + 1013904223u;
        f = &g_frames[(r >> 12) % (unsigned)g_nFrames];
        switch ((r >> 8) % 4u) {
        case 0: w->bad |= decode_check(f, (int)((r >> 16) & 1u), out); break;
        case 1: w->bad |= compress_check(g_data, g_n / 2, 131072, 10, out); break;
        default: w->bad |= dev_decode(f, f->n + ((r >> 17) & 1u ? 77 : 0), (r >> 18) & 1u, f->n, 1); break;
        }
    }
    free(out);
    return NULL;
}
static int devthreads(int n, int rounds)
{
    pthread_t th[64], wd;
    Worker w[64];
    int i, bad = 0;
    if (n > 64) return 2;
    setup(3 * 131072 + 99);
    setenv("LIZARDGPU_WALK_RECORDS", "2", 1);                 /* (before the threads start: the environment is only read from then on) */
    fh_set_schedule(FH_RANDOM, 2424);
    g_syncUpload = 1;
    hipStreamCreateWithFlags(&g_user, hipStreamNonBlocking);
    pthread_create(&wd, NULL, watchdog, NULL); pthread_detach(wd);
    for (i = 0; i < n; i++) { w[i].id = i; w[i].rounds = rounds; w[i].bad = 0; pthread_create(&th[i], NULL, dev_worker, &w[i]); }
    for (i = 0; i < n; i++) { pthread_join(th[i], NULL); bad += w[i].bad; }
    printf("pipeline_fake devthreads: %d threads x %d rounds, %d bad, %llu ops\n", n, rounds, bad, fh_ops_run());
    return bad ? 1 : 0;
}
int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "core")) return core();
    if (argc > 1 && !strcmp(argv[1], "devcore")) return devcore();
    if (argc > 1 && !strcmp(argv[1], "devthreads")) return devthreads(argc > 2 ? atoi(argv[2]) : 6, argc > 3 ? atoi(argv[3]) : 3);
    if (argc > 1 && !strcmp(argv[1], "threads")) return threads(argc > 2 ? atoi(argv[2]) : 8, argc > 3 ? atoi(argv[3]) : 6, argc > 4 ? atoi(argv[4]) : 1);
    fprintf(stderr, "usage: pipeline_fake core | threads [n] [rounds] [big] | devcore | devthreads [n] [rounds]\n");
    return 2;
}
#endif
