/* lizard_planes_device.c — LizardGPU_splitPlanes_device / LizardGPU_joinPlanes_device: the bytes of a batch of device buffers
 * regrouped by significance, and back, in ONE launch each (planes_kernels.h is the device side); LizardGPU_splitBitPlanes_device /
 * LizardGPU_joinBitPlanes_device: the same call with their bits regrouped by weight (bitplanes_kernels.h);
 * LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device: either of them with every buffer XORed with an earlier version of
 * itself, its base, on the way (a table of 40-byte entries and the XOR kernels of the same two headers); and the tensor header — a
 * skippable frame that tells a reader of a stream which filter and element size a frame's bytes were split with, and the tensor's
 * dtype and shape (include/lizard_amd.h Part 3c).  Plain C on the HIP runtime's C API and the shim of lizard_gpu_ctx.h, like the sibling
 * device entries.
 *
 * A call: the arguments are checked before anything is touched; the non-empty buffers become the entries of a table, each with
 * the number of its first tile (planes_kernels.h); the table goes up from pinned memory and the kernel runs, both on the caller's
 * stream, behind what it holds; the host waits once.  The table lives in LzCtx::dfTab and stage 0's pinned buffer, like the
 * tables of the sibling entries: 32 bytes per buffer.  There is no host loop anywhere: no device is an error. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_common.h"
#include "planes_kernels.h"

/* withBases: the table holds LzPlanesXorEntry (the XOR entries), else LzPlanesEntry. */
static int planes_locked(LzCtx* c, const void* tab, size_t nEntries, uint32_t nTiles, int join, int bits, int withBases, hipStream_t stream)
{
    int rc;
    if ((rc = lz_table_upload(c, tab, nEntries * (withBases ? sizeof(LzPlanesXorEntry) : sizeof(LzPlanesEntry)), stream))) return rc;
    rc = withBases ? lzk_planes_xor_launch(c, (const LzPlanesXorEntry*)c->dfTab, (uint32_t)nEntries, nTiles, join, bits, stream)
                   : lzk_planes_launch(c, (const LzPlanesEntry*)c->dfTab, (uint32_t)nEntries, nTiles, join, bits, stream);
    if (rc) return rc;
    LZ_HIP(hipStreamSynchronize(stream));
    return 0;
}

/* bits: 0 = byte planes, 1 = bit planes.  The checks, the tiles and the table are the same for both; the kernel and the counters
 * differ.  withBases: the XOR entries — a table of LzPlanesXorEntry with d_bases[i] (0 where d_bases or d_bases[i] is null), the XOR
 * kernels and counters of their own. */
static int planes(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const void* const* d_bases, const size_t* sizes,
                  const uint32_t* elemSizes, int join, int bits, int withBases, hipStream_t stream)
{
    LzPlanesEntry* tab = NULL;
    LzPlanesXorEntry* xtab = NULL;
    LzGuard g;
    uint64_t tiles = 0, bytes = 0;
    size_t i, live = 0;
    int rc;
    if (!nBuffers) return 0;
    lzk_err()[0] = 0;
    if (!d_dsts || !d_srcs || !sizes || !elemSizes) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null array)"); return -LIZARDGPU_ERR_ARG; }
    for (i = 0; i < nBuffers; i++) {
        const uint32_t E = elemSizes[i];
        if (E != 1 && E != 2 && E != 4 && E != 8) {
            snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (buffer %zu: element size %u is not 1, 2, 4 or 8)", i, (unsigned)E);
            return -LIZARDGPU_ERR_ARG;
        }
        if (!sizes[i]) continue;
        if (!d_dsts[i] || !d_srcs[i]) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (buffer %zu: null pointer)", i); return -LIZARDGPU_ERR_ARG; }
        tiles += sizes[i] < E ? 1 : ((uint64_t)(sizes[i] / E) * E + LZP_TILE_BYTES - 1) / LZP_TILE_BYTES;
        live++;
    }
    if (tiles >> 32) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (the batch has 2^32 tiles of %u bytes or more)", LZP_TILE_BYTES); return -LIZARDGPU_ERR_ARG; }
    if (!live) return 0;                                        /* nothing but empty buffers: nothing to move */
    if (withBases) xtab = (LzPlanesXorEntry*)malloc(live * sizeof *xtab);
    else tab = (LzPlanesEntry*)malloc(live * sizeof *tab);
    if (!tab && !xtab) { snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); return -LIZARDGPU_ERR_NOMEM; }
    for (i = 0, live = 0, tiles = 0; i < nBuffers; i++) {
        const uint32_t E = elemSizes[i];
        if (!sizes[i]) continue;
        if (withBases) {
            xtab[live].src = (uint64_t)(uintptr_t)d_srcs[i]; xtab[live].dst = (uint64_t)(uintptr_t)d_dsts[i];
            xtab[live].base = d_bases ? (uint64_t)(uintptr_t)d_bases[i] : 0; xtab[live].size = (uint64_t)sizes[i];
            xtab[live].elem = E; xtab[live].firstTile = (uint32_t)tiles;
        } else {
            tab[live].src = (uint64_t)(uintptr_t)d_srcs[i]; tab[live].dst = (uint64_t)(uintptr_t)d_dsts[i]; tab[live].size = (uint64_t)sizes[i];
            tab[live].elem = E; tab[live].firstTile = (uint32_t)tiles;
        }
        tiles += sizes[i] < E ? 1 : ((uint64_t)(sizes[i] / E) * E + LZP_TILE_BYTES - 1) / LZP_TILE_BYTES;
        bytes += sizes[i];
        live++;
    }
    lzk_guard_acquire(&g);
    if (g.rc) { free(tab); free(xtab); return g.rc; }
    rc = planes_locked(g.c, withBases ? (const void*)xtab : (const void*)tab, live, (uint32_t)tiles, join, bits, withBases, stream);
    if (rc) lz_drain_caller(stream);
    else {
        unsigned long long* const st = withBases ? g.c->devPlanesXorStats : bits ? g.c->devBitPlanesStats : g.c->devPlanesStats;
        st[join ? 1 : 0] += nBuffers;
        st[2] += bytes;
        st[3]++;
    }
    lzk_guard_release(&g);
    free(tab);
    free(xtab);
    return rc;
}

int LizardGPU_splitPlanes_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const size_t* sizes,
                                 const uint32_t* elemSizes, void* stream)
{
    return planes(nBuffers, d_dsts, d_srcs, NULL, sizes, elemSizes, 0, 0, 0, (hipStream_t)stream);
}

int LizardGPU_joinPlanes_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const size_t* sizes,
                                const uint32_t* elemSizes, void* stream)
{
    return planes(nBuffers, d_dsts, d_srcs, NULL, sizes, elemSizes, 1, 0, 0, (hipStream_t)stream);
}

int LizardGPU_planesStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devPlanesStats));
}

int LizardGPU_splitBitPlanes_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const size_t* sizes,
                                    const uint32_t* elemSizes, void* stream)
{
    return planes(nBuffers, d_dsts, d_srcs, NULL, sizes, elemSizes, 0, 1, 0, (hipStream_t)stream);
}

int LizardGPU_joinBitPlanes_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const size_t* sizes,
                                   const uint32_t* elemSizes, void* stream)
{
    return planes(nBuffers, d_dsts, d_srcs, NULL, sizes, elemSizes, 1, 1, 0, (hipStream_t)stream);
}

int LizardGPU_bitPlanesStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devBitPlanesStats));
}

/* The XOR entries: `filter` chooses the layout.  A filter that is neither is refused before anything else is looked at. */
static int planes_xor(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const void* const* d_bases, const size_t* sizes,
                      const uint32_t* elemSizes, unsigned filter, int join, hipStream_t stream)
{
    if (filter != LIZARDGPU_FILTER_BYTE_PLANES && filter != LIZARDGPU_FILTER_BIT_PLANES) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (filter %u is neither byte planes nor bit planes)", filter);
        return -LIZARDGPU_ERR_ARG;
    }
    return planes(nBuffers, d_dsts, d_srcs, d_bases, sizes, elemSizes, join, filter == LIZARDGPU_FILTER_BIT_PLANES, 1, stream);
}

int LizardGPU_splitPlanesXor_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const void* const* d_bases,
                                    const size_t* sizes, const uint32_t* elemSizes, unsigned filter, void* stream)
{
    return planes_xor(nBuffers, d_dsts, d_srcs, d_bases, sizes, elemSizes, filter, 0, (hipStream_t)stream);
}

int LizardGPU_joinPlanesXor_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const void* const* d_bases,
                                   const size_t* sizes, const uint32_t* elemSizes, unsigned filter, void* stream)
{
    return planes_xor(nBuffers, d_dsts, d_srcs, d_bases, sizes, elemSizes, filter, 1, (hipStream_t)stream);
}

int LizardGPU_planesXorStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devPlanesXorStats));
}

/* ---- the tensor header: host code, no device ---- */
#define LZT_FIXED 40                                           /* payload bytes in front of the dims */

static void put_le(uint8_t* p, uint64_t v, int n) { int i; for (i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static uint64_t get_le(const uint8_t* p, int n) { uint64_t v = 0; int i; for (i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i); return v; }
static int elem_ok(uint32_t e) { return e == 1 || e == 2 || e == 4 || e == 8; }

/* Both versions: the v1 fields of the descriptor and the filter.  "LZT1" is filter 0 with zero pad bytes; "LZT2" holds the filter
 * in payload byte 6 and is written for a filter other than 0 only, so that every meaning has one encoding. */
static size_t header_write(void* dst, size_t dstCapacity, const LizardGPU_tensorDesc_t* desc, uint32_t filter)
{
    uint8_t* p = (uint8_t*)dst;
    size_t total;
    uint32_t i;
    if (!dst || !desc || !elem_ok(desc->elemSize) || desc->ndim > 8 || !memchr(desc->dtype, 0, sizeof desc->dtype)) return 0;
    if (filter != LIZARDGPU_FILTER_BYTE_PLANES && filter != LIZARDGPU_FILTER_BIT_PLANES) return 0;
    total = 8 + LZT_FIXED + 8 * (size_t)desc->ndim;
    if (dstCapacity < total) return 0;
    put_le(p, LIZARDGPU_TENSOR_MAGIC, 4);
    put_le(p + 4, total - 8, 4);
    memcpy(p + 8, filter ? "LZT2" : "LZT1", 4);
    p[12] = (uint8_t)desc->elemSize; p[13] = (uint8_t)desc->ndim; p[14] = (uint8_t)filter; p[15] = 0;
    put_le(p + 16, desc->nbytes, 8);
    memset(p + 24, 0, 24);
    memcpy(p + 24, desc->dtype, strlen(desc->dtype));
    for (i = 0; i < desc->ndim; i++) put_le(p + 8 + LZT_FIXED + 8 * i, desc->shape[i], 8);
    return total;
}

size_t LizardGPU_tensorHeaderWrite(void* dst, size_t dstCapacity, const LizardGPU_tensorDesc_t* desc)
{
    return header_write(dst, dstCapacity, desc, LIZARDGPU_FILTER_BYTE_PLANES);
}

size_t LizardGPU_tensorHeaderWrite2(void* dst, size_t dstCapacity, const LizardGPU_tensorDesc2_t* desc)
{
    LizardGPU_tensorDesc_t v1;
    if (!desc) return 0;
    memcpy(&v1, desc, sizeof v1);                              /* the v1 fields come first */
    return header_write(dst, dstCapacity, &v1, desc->filter);
}

/* "LZT3": the tensor's bytes were XORed with a base before the filter.  The "LZT2" layout with payload byte 7 = the flags (1), the
 * base's tag behind the dtype and the dims behind that. */
#define LZT3_FIXED 48

size_t LizardGPU_tensorHeaderWrite3(void* dst, size_t dstCapacity, const LizardGPU_tensorDesc3_t* desc)
{
    uint8_t* p = (uint8_t*)dst;
    size_t total;
    uint32_t i;
    if (!desc) return 0;
    if (desc->flags == 0) {                                    /* no base: "LZT1" / "LZT2", so that every meaning has one encoding */
        LizardGPU_tensorDesc_t v1;
        if (desc->baseTag) return 0;
        memcpy(&v1, desc, sizeof v1);
        return header_write(dst, dstCapacity, &v1, desc->filter);
    }
    if (desc->flags != LIZARDGPU_TENSOR_XOR_BASE) return 0;
    if (!dst || !elem_ok(desc->elemSize) || desc->ndim > 8 || !memchr(desc->dtype, 0, sizeof desc->dtype)) return 0;
    if (desc->filter != LIZARDGPU_FILTER_BYTE_PLANES && desc->filter != LIZARDGPU_FILTER_BIT_PLANES) return 0;
    total = 8 + LZT3_FIXED + 8 * (size_t)desc->ndim;
    if (dstCapacity < total) return 0;
    put_le(p, LIZARDGPU_TENSOR_MAGIC, 4);
    put_le(p + 4, total - 8, 4);
    memcpy(p + 8, "LZT3", 4);
    p[12] = (uint8_t)desc->elemSize; p[13] = (uint8_t)desc->ndim; p[14] = (uint8_t)desc->filter; p[15] = (uint8_t)desc->flags;
    put_le(p + 16, desc->nbytes, 8);
    memset(p + 24, 0, 24);
    memcpy(p + 24, desc->dtype, strlen(desc->dtype));
    put_le(p + 48, desc->baseTag, 8);
    for (i = 0; i < desc->ndim; i++) put_le(p + 8 + LZT3_FIXED + 8 * i, desc->shape[i], 8);
    return total;
}

/* ver: the reader's version — 1 knows "LZT1" only, 2 "LZT2" as well, 3 all three tags.  *filter, *flags and *baseTag are written
 * together with *desc. */
static int header_read(const void* src, size_t srcSize, LizardGPU_tensorDesc_t* desc, uint32_t* filter, uint32_t* flags, uint64_t* baseTag,
                       size_t* headerBytes, int ver)
{
    const uint8_t* p = (const uint8_t*)src;
    int tag = 1;                                               /* the digit of "LZTn"; known once 12 bytes are in hand */
    const int unknown = -(int)LIZARDGPU_FRAME_ERR_frameType_unknown, incomplete = -(int)LIZARDGPU_FRAME_ERR_frameHeader_incomplete;
    const uint64_t widest = ver >= 3 ? LZT3_FIXED : LZT_FIXED; /* the largest fixed part of a tag this reader knows */
    uint64_t len, fixed = LZT_FIXED;
    uint32_t ndim = 0, i;
    if (headerBytes) *headerBytes = 0;
    if (!src && srcSize) return -(int)LIZARDGPU_FRAME_ERR_GENERIC;
    /* every field is judged as soon as the bytes in hand hold it: a prefix of a header is incomplete, never unknown */
    if (srcSize < 4) return incomplete;
    if (get_le(p, 4) != LIZARDGPU_TENSOR_MAGIC) return unknown;
    if (srcSize < 8) return incomplete;
    len = get_le(p + 4, 4);
    if (len < LZT_FIXED || len > widest + 64 || (len - LZT_FIXED) % 8) return unknown;   /* a length of some tag this reader knows */
    if (srcSize >= 12) {
        if (!memcmp(p + 8, "LZT1", 4)) tag = 1;
        else if (ver >= 2 && !memcmp(p + 8, "LZT2", 4)) tag = 2;
        else if (ver >= 3 && !memcmp(p + 8, "LZT3", 4)) tag = 3;
        else return unknown;
        fixed = tag == 3 ? LZT3_FIXED : LZT_FIXED;
        if (len < fixed || len > fixed + 64) return unknown;    /* ... and of this tag */
        ndim = (uint32_t)(len - fixed) / 8;
    }
    if (srcSize >= 13 && !elem_ok(p[12])) return unknown;
    if (srcSize >= 14 && p[13] != ndim) return unknown;
    if (srcSize >= 15 && (tag == 3 ? p[14] > LIZARDGPU_FILTER_BIT_PLANES : p[14] != (tag == 2 ? LIZARDGPU_FILTER_BIT_PLANES : 0))) return unknown;
    if (srcSize >= 16 && p[15] != (tag == 3 ? LIZARDGPU_TENSOR_XOR_BASE : 0)) return unknown;
    if (srcSize >= 48 && !memchr(p + 24, 0, 24)) return unknown;
    if (srcSize < 8 + len) return incomplete;
    if (desc) {
        memset(desc, 0, sizeof *desc);
        desc->elemSize = p[12]; desc->ndim = ndim; desc->nbytes = get_le(p + 16, 8);
        memcpy(desc->dtype, p + 24, 24);
        for (i = 0; i < ndim; i++) desc->shape[i] = get_le(p + 8 + fixed + 8 * i, 8);
    }
    if (filter) *filter = p[14];
    if (flags) *flags = p[15];
    if (baseTag) *baseTag = tag == 3 ? get_le(p + 48, 8) : 0;
    if (headerBytes) *headerBytes = (size_t)(8 + len);
    return 0;
}

int LizardGPU_tensorHeaderRead(const void* src, size_t srcSize, LizardGPU_tensorDesc_t* desc, size_t* headerBytes)
{
    return header_read(src, srcSize, desc, NULL, NULL, NULL, headerBytes, 1);
}

int LizardGPU_tensorHeaderRead2(const void* src, size_t srcSize, LizardGPU_tensorDesc2_t* desc, size_t* headerBytes)
{
    LizardGPU_tensorDesc_t v1;
    uint32_t filter = 0;
    const int rc = header_read(src, srcSize, &v1, &filter, NULL, NULL, headerBytes, 2);
    if (!rc && desc) {
        memcpy(desc, &v1, sizeof v1);
        desc->filter = filter; desc->reserved = 0;
    }
    return rc;
}

int LizardGPU_tensorHeaderRead3(const void* src, size_t srcSize, LizardGPU_tensorDesc3_t* desc, size_t* headerBytes)
{
    LizardGPU_tensorDesc_t v1;
    uint32_t filter = 0, flags = 0;
    uint64_t baseTag = 0;
    const int rc = header_read(src, srcSize, &v1, &filter, &flags, &baseTag, headerBytes, 3);
    if (!rc && desc) {
        memcpy(desc, &v1, sizeof v1);
        desc->filter = filter; desc->flags = flags; desc->baseTag = baseTag;
    }
    return rc;
}
