/* tests/seek_device_fake.c — TEST INFRASTRUCTURE: the READERS of lizard_amd/csrc/lizard_seek_device.c (LizardGPU_seekTable_device,
 * LizardGPU_decompressSeekableStream_device, LizardGPU_decompressStreamItems_device) compiled as a unit under test on a CPU, on the fake
 * HIP runtime with DEFERRED streams.  Linked with tests/unstream_device_fake.c (LizardGPU_decompressStream_device, the entry the unit
 * must equal and falls back to), tests/unframes_device_fake.c (the batch decoder), tests/pipeline_fake.c, tests/fake_hip.c and
 * lizard_amd/csrc/lizard_seek_host.c as they are.  ssf_run decodes one caller-given stream through both whole-stream entries on the
 * same fake and compares the answers — return value, consumed bytes, frame count, decoded count, the decoded bytes, the canary
 * margins.  The unit's WRITER needs lizard_stream_device.c and the table kernel, which have harnesses of their own
 * (tests/stream_device_fake.c, tests/emul/seektable_api.cpp); here its two seams answer "not in this harness". */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../lizard_amd/csrc/lizard_seek_device.c"            /* unit under test, compiled into this harness */
#include "device_fake_common.h"

size_t lzgpu_stream_compress(void* d_dst, size_t dstCapacity, size_t nFrames, const void* const* d_srcs, const size_t* srcSizes,
                             const void* const* prefixes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs, uint64_t* frameOffsets,
                             size_t* failedFrame, void* stream, uint64_t extraFixed, lzgpu_stream_after_fn after, void* afterArg)
{
    (void)d_dst; (void)dstCapacity; (void)nFrames; (void)d_srcs; (void)srcSizes; (void)prefixes; (void)prefixSizes; (void)prefs; (void)frameOffsets;
    (void)failedFrame; (void)stream; (void)extraFixed; (void)after; (void)afterArg;
    snprintf(lzk_err(), LZK_ERR_BYTES, "lzgpu_stream_compress: not in this harness");
    return LZ_FRAME_E(GENERIC);
}
int lzk_stream_seektable_launch(const LzFramesEntry* d_frames, const LzStreamEntry* d_entries, const LzStreamState* d_state, const uint64_t* d_offsets,
                                uint32_t nFrames, uint64_t fixedTotal, uint64_t capacity, hipStream_t stream)
{
    (void)d_frames; (void)d_entries; (void)d_state; (void)d_offsets; (void)nFrames; (void)fixedTotal; (void)capacity; (void)stream;
    snprintf(lzk_err(), LZK_ERR_BYTES, "lzk_stream_seektable_launch: not in this harness");
    return -LIZARDGPU_ERR_HIP;
}

const char* ssf_last_error(void) { return dfc_text; }           /* LizardGPU_lastError as the seekable entry left it */

/* The stream `bytes` through LizardGPU_decompressStream_device and through LizardGPU_decompressSeekableStream_device, cap bytes of room
 * each.  0 when the two answers are one; got: the seekable entry's return value, consumed, frames, decoded, then the growth of
 * LizardGPU_seekDeviceStats [0..3] over its call. */
int ssf_run(const uint8_t* bytes, size_t n, size_t cap, unsigned flags, unsigned skew, unsigned long long got[8])
{
    Region src, a, b;
    unsigned long long s0[4], s1[4];
    size_t ra, rb, ua = 111, ub = 222, fa = 111, fb = 222, da = 111, db = 222;
    const hipStream_t user = dfc_user();
    int bad = 0, g;
    if (region_make(&src, bytes, n, skew & 7, 0x5A) || region_make(&a, NULL, cap, (skew * 3) & 7, 0xC3) || region_make(&b, NULL, cap, (skew * 5) & 7, 0xC3)) return 100;
    ra = LizardGPU_decompressStream_device(region_at(&a), cap, region_at(&src), n, &ua, &fa, &da, flags, user);
    LizardGPU_seekDeviceStats(s0);
    rb = LizardGPU_decompressSeekableStream_device(region_at(&b), cap, region_at(&src), n, &ub, &fb, &db, flags, user);
    dfc_keep_text();
    LizardGPU_seekDeviceStats(s1);
    hipStreamSynchronize(user);
    if (got) { got[0] = rb; got[1] = ub; got[2] = fb; got[3] = db; for (g = 0; g < 4; g++) got[4 + g] = s1[g] - s0[g]; }
    if (region_fetch_same(&src, bytes) || region_fetch(&a) || region_fetch(&b)) bad = 1;
    if (!bad && (ra != rb || ua != ub || fa != fb || da != db)) bad = 2;
    if (!bad && da && memcmp(region_bytes(&a), region_bytes(&b), da)) bad = 3;
    if (bad) fprintf(stderr, "seek_device_fake: %s (walk: %zu, consumed %zu, %zu frames, %zu decoded; seekable: %zu, consumed %zu, %zu frames, %zu decoded; %zu bytes, cap %zu): %s\n",
                     bad == 1 ? "a canary margin or the source changed" : bad == 2 ? "the answers differ" : "the decoded bytes differ", ra, ua, fa, da, rb, ub, fb,
                     db, n, cap, dfc_text);
    region_free(&src); region_free(&a); region_free(&b);
    return bad;
}

/* LizardGPU_decompressStreamItems_device over the stream into cap bytes: the return value; the bytes come back in out[0 .. cap) */
size_t ssf_items(const uint8_t* bytes, size_t n, size_t cap, const size_t* items, size_t nItems, uint64_t* itemOffsets, size_t* failedItem, uint8_t* out)
{
    Region src, d;
    const hipStream_t user = dfc_user();
    size_t r;
    if (region_make(&src, bytes, n, 3, 0x5A) || region_make(&d, NULL, cap, 5, 0xC3)) return LZ_FRAME_E(allocation_failed);
    r = LizardGPU_decompressStreamItems_device(region_at(&d), cap, region_at(&src), n, items, nItems, itemOffsets, failedItem, 0, user);
    dfc_keep_text();
    hipStreamSynchronize(user);
    if (region_fetch(&src) || region_fetch(&d)) r = LZ_FRAME_E(maxCode);
    else if (cap) memcpy(out, region_bytes(&d), cap);
    region_free(&src); region_free(&d);
    return r;
}
