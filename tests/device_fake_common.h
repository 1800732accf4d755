/* tests/device_fake_common.h — TEST INFRASTRUCTURE: what the harnesses that run a host file of lizard_amd/csrc on the fake HIP runtime
 * (the tests/..._device_fake.c files and tests/pipeline_fake.c) share.  Included behind the unit under test.  Static functions and
 * variables only: the harnesses are linked together in several combinations, and each keeps a copy of its own (its own caller's
 * stream, its own saved error text, its own refusal counters); a file takes what it uses. */
#ifndef DEVICE_FAKE_COMMON_H
#define DEVICE_FAKE_COMMON_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../lizard_amd/csrc/lizard_device_common.h"
#include "../lizard_amd/csrc/lizard_gpu_shim.h"
#include "../lizard_amd/csrc/lizard_xxhash.h"
#include "fake_hip.h"

/* a harness function answers 1 with "<name>: line N: <text>" on stderr; a file defines CHECK(cond, ...) with its name */
#define DFC_CHECK(name, cond, ...) do { if (!(cond)) { fprintf(stderr, name ": line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

/* ---- the caller's stream, made at its first use, and LizardGPU_lastError as the call under test left it ---- */
static hipStream_t dfc_stream;
static inline hipStream_t dfc_user(void)
{
    if (!dfc_stream) hipStreamCreateWithFlags(&dfc_stream, hipStreamNonBlocking);
    return dfc_stream;
}
static char dfc_text[LZK_ERR_BYTES];
static inline void dfc_keep_text(void) { snprintf(dfc_text, sizeof dfc_text, "%s", LizardGPU_lastError()); }

/* ---- "the n-th launch of that kind from now answers -LIZARDGPU_ERR_HIP, once, and enqueues nothing" ---- */
#define DFC_KINDS 8
static int dfc_refuse[DFC_KINDS];
static inline void dfc_refuse_set(int kind, int nth)           /* under the context guard: a launch counts down under it */
{
    LzGuard g;
    lzk_guard_acquire(&g);
    if (kind >= 0 && kind < DFC_KINDS) dfc_refuse[kind] = nth;
    lzk_guard_release(&g);
}
static inline int dfc_refused(int kind, const char* what)      /* in a launch shim: 1 with the error text when this launch is the one */
{
    if (!dfc_refuse[kind] || --dfc_refuse[kind]) return 0;
    snprintf(lzk_err(), LZK_ERR_BYTES, "%s: refused by the test", what);
    return 1;
}

/* ---- the order in which the waves of a launch claim its n work items ---- */
static inline void dfc_shuffled(uint32_t* order, size_t n)
{
    size_t i;
    for (i = 0; i < n; i++) order[i] = (uint32_t)i;
    for (i = n; i > 1; i--) { const size_t k = fh_rand() % i; const uint32_t t = order[i - 1]; order[i - 1] = order[k]; order[k] = t; }
}

/* ---- the canary region: n bytes in device memory between two margins of `fill`, with a pinned twin ---- */
#define DFC_G 4096                                            /* the margin in front; DFC_G + 8 - skew bytes behind: a skew of 0 .. 7 leaves a checked tail */
typedef struct { uint8_t *dev, *host; size_t n, skew; uint8_t fill; } Region;
static inline size_t region_all(const Region* r) { return r->n + 2 * DFC_G + 8; }
/* n bytes from `bytes` (or of `fill`), skew bytes off the 4 KiB margin, uploaded on the caller's stream, not waited for */
static inline int region_make(Region* r, const uint8_t* bytes, size_t n, size_t skew, uint8_t fill)
{
    r->n = n; r->skew = skew; r->fill = fill;
    if (hipMalloc((void**)&r->dev, region_all(r)) != hipSuccess || hipHostMalloc((void**)&r->host, region_all(r), 0) != hipSuccess) return 1;
    memset(r->host, fill, region_all(r));
    if (bytes && n) memcpy(r->host + DFC_G + skew, bytes, n);
    return hipMemcpyAsync(r->dev, r->host, region_all(r), hipMemcpyHostToDevice, dfc_user()) != hipSuccess;
}
static inline uint8_t* region_at(const Region* r) { return r->dev + DFC_G + r->skew; }             /* the bytes, in device memory */
static inline uint8_t* region_bytes(const Region* r) { return r->host + DFC_G + r->skew; }         /* ... and behind region_fetch in the twin */
/* downloads; 0 when both margins hold `fill` */
static inline int region_fetch(Region* r)
{
    size_t q;
    memset(r->host, 0, region_all(r));
    if (hipMemcpy(r->host, r->dev, region_all(r), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    for (q = 0; q < DFC_G + r->skew; q++) if (r->host[q] != r->fill) return 1;
    for (q = DFC_G + r->skew + r->n; q < region_all(r); q++) if (r->host[q] != r->fill) return 1;
    return 0;
}
/* region_fetch, and the bytes are still `bytes` (a source the call must not have touched) */
static inline int region_fetch_same(Region* r, const uint8_t* bytes) { return region_fetch(r) || (r->n && memcmp(region_bytes(r), bytes, r->n)); }
static inline void region_free(Region* r) { hipFree(r->dev); hipHostFree(r->host); }

/* ---- lz_xxh32_frames_kernel: every live entry that asks for a checksum gets the XXH32 of its source; the body of a harness's
 * lzk_frames_hash_launch ---- */
typedef struct { LzFramesEntry* frames; uint32_t n; } DfcHashK;
static inline void dfc_frames_hash_kernel(void* a)
{
    const DfcHashK* k = (const DfcHashK*)a;
    const uint32_t want = LZK_FRAMES_LIVE | LZK_FRAMES_CHECKSUM;
    uint32_t f;
    if (!fh_check_dev(k->frames, (size_t)k->n * sizeof *k->frames, "frames hash: the frame table")) return;
    for (f = 0; f < k->n; f++) {
        LzFramesEntry* e = k->frames + f;
        if ((e->flags & want) != want) continue;
        if (e->srcSize && !fh_check_dev((const void*)(uintptr_t)e->src, (size_t)e->srcSize, "frames hash: a frame's source")) continue;
        e->hash = Lizard_XXH32((const void*)(uintptr_t)e->src, (size_t)e->srcSize, 0);
    }
}
static inline int dfc_frames_hash_launch(LzFramesEntry* d_frames, uint32_t nFrames, hipStream_t stream)
{
    DfcHashK k;
    if (!d_frames || nFrames == 0) { snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_frames_hash_launch: bad argument"); return -LIZARDGPU_ERR_ARG; }
    k.frames = d_frames; k.n = nFrames;
    return fh_enqueue_kernel(stream, dfc_frames_hash_kernel, &k, sizeof k) == hipSuccess ? 0 : -LIZARDGPU_ERR_HIP;
}

#endif
