/* tests/frame_device_fake.c — TEST INFRASTRUCTURE: lizard_amd/csrc/lizard_frame_device.c (LizardGPU_compressFrame_device: all chunks
 * enqueued up front on three streams, the stages' slots rotating under events, the cursor carried in device memory, the checksum pass
 * over the source) compiled as a unit under test on a CPU, on the fake HIP runtime with DEFERRED streams.  Linked with
 * tests/pipeline_fake.c (the context, lzk_launch = the oracle as the block kernels, the host twin LizardGPU_compressFrame on the same
 * fake) and tests/fake_hip.c as they are; this file adds the one shim they do not have: lzk_frame_pack_launch, a plain sequential
 * model of lz_frame_scan_kernel + lz_frame_gather_kernel (lz_frame_pack.h) that checks that everything it touches lies in live device
 * memory.  pf_refuse_frame_pack: the n-th such launch from now answers -LIZARDGPU_ERR_HIP, once, and enqueues nothing (what
 * pf_refuse_launch is to the decoder's launches).
 *   library : with pipeline_fake.c, -shared (tests/test_frame_compress_fake_device.py drives it through ctypes)
 *   program : -DFRAME_DEVICE_FAKE_MAIN, for the sanitizer build: exit 0 = all good */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../lizard_amd/csrc/lizard_frame_device.c"        /* unit under test, compiled into this harness */
#include "device_fake_common.h"

void pf_refuse_frame_pack(int nth) { dfc_refuse_set(0, nth); }

typedef struct { const uint8_t *in, *slots; size_t slot; const uint32_t* sizes; uint64_t* offsets; uint8_t* dst; uint32_t nb, blockSize, last; uint64_t* state; uint64_t limit; } FramePackK;
static void frame_pack_kernel(void* a)
{
    const FramePackK* k = (const FramePackK*)a;
    uint64_t run, raw = 0;
    uint32_t b;
    if (!fh_check_dev(k->sizes, 4 * (size_t)k->nb, "frame pack: sizes") || !fh_check_dev(k->offsets, 8 * (size_t)k->nb, "frame pack: offsets")
        || !fh_check_dev(k->state, 32, "frame pack: state")) return;
    run = k->state[0];
    for (b = 0; b < k->nb; b++) {
        const uint32_t n = b == k->nb - 1u ? k->last : k->blockSize, cs = k->sizes[b];
        const int isRaw = n != 1u && (cs == 0u || cs > n - 1u);
        const uint32_t len = isRaw ? n : cs, word = isRaw ? (n | 0x80000000u) : cs;
        const uint8_t* from = isRaw ? k->in + (size_t)b * k->blockSize : k->slots + (size_t)b * k->slot;
        k->offsets[b] = run;
        raw += (uint64_t)isRaw;
        if (run <= k->limit && k->limit - run >= 4ull + len && fh_check_dev(k->dst + run, 4 + (size_t)len, "frame pack: a record's place in d_dst")
            && (!len || fh_check_dev(from, len, "frame pack: a record's source"))) {
            uint8_t* out = k->dst + run;
            out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
            if (len) memcpy(out + 4, from, len);
        }
        run += 4ull + len;
    }
    k->state[0] = run;
    if (run > k->limit) k->state[1] = 1;
    k->state[2] += raw;
}
int lzk_frame_pack_launch(const void* d_in, const void* d_slots, size_t slot, const uint32_t* d_sizes, uint64_t* d_offsets, void* d_dst,
                          uint32_t nb, uint32_t blockSize, uint32_t lastBlockSize, uint64_t* d_state, uint64_t limit, hipStream_t stream)
{
    FramePackK k;
    if (!d_in || !d_slots || !d_sizes || !d_offsets || !d_dst || !d_state || nb == 0 || blockSize == 0 || lastBlockSize == 0 || lastBlockSize > blockSize) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_frame_pack_launch: bad argument"); return -LIZARDGPU_ERR_ARG;
    }
    if (dfc_refused(0, "lzk_frame_pack_launch")) return -LIZARDGPU_ERR_HIP;
    k.in = (const uint8_t*)d_in; k.slots = (const uint8_t*)d_slots; k.slot = slot; k.sizes = d_sizes; k.offsets = d_offsets; k.dst = (uint8_t*)d_dst;
    k.nb = nb; k.blockSize = blockSize; k.last = lastBlockSize; k.state = d_state; k.limit = limit;
    return fh_enqueue_kernel(stream, frame_pack_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

#ifdef FRAME_DEVICE_FAKE_MAIN
/* ---- the program form, for the sanitizer build: device entry = host twin over schedules, chunkings and capacities ---- */
#include "lizard_oracle.h"
void pf_set_chunk_bytes(size_t n);
void pf_shutdown(void);
#define CHECK(cond, ...) DFC_CHECK("frame_device_fake", cond, __VA_ARGS__)
static int g_failMalloc;          /* the n-th hipMalloc inside the next device call fails */

/* both entries on the same bytes: the same answer, the same frame, the margins of d_dst and d_src untouched.  capDelta: capacity
 * relative to the bound.  want: (size_t)0 = whatever the twin says, a size or an error; else that error (the twin too, unless it is
 * GENERIC: a failure of the machinery that the test provoked in the device entry alone) */
static int both(const uint8_t* data, size_t n, int level, int bsid, int checksum, int csize, long capDelta, size_t want)
{
    LizardF_preferences_t p;
    const hipStream_t user = dfc_user();
    Region src, dst;
    uint8_t* twin;
    size_t bound, cap, r, t;
    int bad = 0;
    memset(&p, 0, sizeof p);
    p.frameInfo.blockSizeID = (LizardF_blockSizeID_t)bsid; p.frameInfo.blockMode = (LizardF_blockMode_t)1;
    p.frameInfo.contentChecksumFlag = (LizardF_contentChecksum_t)checksum; p.frameInfo.contentSize = csize ? n : 0; p.compressionLevel = level;
    bound = LizardGPU_compressFrameBound(n, &p);
    cap = (size_t)((long)bound + capDelta);
    twin = (uint8_t*)malloc(cap + 1);
    CHECK(!region_make(&src, data, n, 0, 0x5A) && !region_make(&dst, NULL, cap, 0, 0xC3), "allocation");
    if (g_failMalloc) hipStreamSynchronize(user);        /* (a call that fails before it orders itself behind the caller's stream leaves that stream's work queued, as it may) */
    fh_fail_malloc(g_failMalloc);
    r = LizardGPU_compressFrame_device(region_at(&dst), cap, region_at(&src), n, &p, user);
    fh_fail_malloc(0); g_failMalloc = 0;
    t = LizardGPU_compressFrame(twin, cap, data, n, &p);
    hipStreamSynchronize(user);                          /* (a call refused up front never touched the caller's stream: the uploads may still be queued) */
    if (region_fetch(&dst) || region_fetch_same(&src, data)) bad = 1;
    if (!bad && want == (size_t)0 && r != t) bad = 2;
    if (!bad && want != (size_t)0 && (r != want || (want != LZ_FRAME_E(GENERIC) && t != want))) bad = 2;
    if (!bad && !LizardF_isError(r) && memcmp(region_bytes(&dst), twin, r)) bad = 3;
    region_free(&src); region_free(&dst); free(twin);
    CHECK(!bad, "compressFrame_device: %s (result %zu, twin %zu, wanted %zu; n %zu level %d checksum %d csize %d cap %zu): %s",
          bad == 1 ? "a canary margin or the source changed" : bad == 2 ? "unexpected result" : "frame bytes differ from the twin's",
          r, t, want, n, level, checksum, csize, cap, LizardGPU_lastError());
    return 0;
}

int main(void)
{
    static const struct { int mode; unsigned seed; } sched[] = { { FH_EAGER, 1 }, { FH_LAZY, 1 }, { FH_RANDOM, 11 }, { FH_RANDOM, 12 }, { FH_RANDOM, 13 } };
    static const char* const chunk[] = { "1", "2", NULL, "4", "1" };
    const size_t bs = 131072, n = 6 * bs + 777;
    uint8_t* data = (uint8_t*)malloc(n);
    size_t s;
    lzo_datagen(data, n, 0.5, 0.0, 77u);
    {   /* noise across a block border: raw records between compressed ones */
        unsigned long long x = 0x9E3779B97F4A7C15ull;
        size_t i;
        for (i = 2 * bs - 5000; i < 3 * bs + 4000; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; data[i] = (uint8_t)(x >> 32); }
    }
    for (s = 0; s < sizeof sched / sizeof sched[0]; s++) {
        const int checksum = (int)(s & 1), level = s & 2 ? 30 : 10;
        fh_set_schedule(sched[s].mode, sched[s].seed);
        pf_set_chunk_bytes((size_t)256 << 10);                        /* unset: two blocks per chunk */
        if (chunk[s]) setenv("LIZARDGPU_FRAME_CHUNK_BLOCKS", chunk[s], 1); else unsetenv("LIZARDGPU_FRAME_CHUNK_BLOCKS");
        if (s == 1) pf_shutdown();
        if (both(data, n, level, 1, checksum, 1, 0, (size_t)0) || both(data, 6 * bs, level, 1, !checksum, 0, 77, (size_t)0)
            || both(data, 3 * bs + 1, level, 1, checksum, 0, 0, (size_t)0) || both(data, 0, level, 0, checksum, 1, 0, (size_t)0)
            || both(data, 1, level, 0, checksum, 0, 0, (size_t)0)) return 1;
        /* capacity: below the bound; the 1-byte last block at exactly the bound under a content-size header, alone and behind a raw block */
        if (both(data, n, level, 1, checksum, 1, -1, LZ_FRAME_E(dstMaxSize_tooSmall)) || both(data, 1, level, 0, 0, 1, 0, LZ_FRAME_E(dstMaxSize_tooSmall))
            || both(data + 2 * bs, bs + 1, level, 1, 0, 1, 0, LZ_FRAME_E(dstMaxSize_tooSmall)) || both(data + 2 * bs, bs + 1, level, 1, 0, 1, 1, (size_t)0)) return 1;
        /* a refused launch, a failing allocation (fresh stages: the first hipMalloc of the call); then a good call */
        pf_refuse_frame_pack(s & 1 ? 2 : 1);
        if (both(data, n, level, 1, checksum, 0, 0, LZ_FRAME_E(GENERIC))) return 1;
        pf_shutdown();
        g_failMalloc = 1 + (int)(s % 3);
        if (both(data, n, level, 1, checksum, 0, 0, LZ_FRAME_E(GENERIC))) return 1;
        if (both(data, n, level, 1, checksum, 0, 0, (size_t)0)) return 1;
    }
    unsetenv("LIZARDGPU_FRAME_CHUNK_BLOCKS");
    free(data);
    printf("frame_device_fake: ok, %llu ops\n", fh_ops_run());
    return 0;
}
#endif
