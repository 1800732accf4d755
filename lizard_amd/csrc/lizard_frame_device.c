/* lizard_frame_device.c — LizardGPU_compressFrame_device: one Lizard frame for bytes that already lie in device memory, written into
 * device memory (include/lizard_amd.h Part 3).  Plain C on the HIP runtime's C API and the shim of lizard_gpu_ctx.h, like
 * lizard_unframe_device.c, whose producing counterpart it is.  It answers what LizardGPU_compressFrame (lizard_frame_host.c,
 * compress_frame with strict = 1) answers for the same bytes, preferences and capacity: the refusals are made here in that function's
 * order by lzgpu_frame_device_plan of that file (which LizardGPU_compressFrames_device, lizard_frames_device.c, calls per frame too), the
 * header is lzgpu_frame_write_header's, the records are what lzgpu_frame_records packs.
 *
 * No payload byte crosses PCIe.  The input is cut into chunks of whole blocks (lzp_chunk_bytes; LIZARDGPU_FRAME_CHUNK_BLOCKS
 * overrides the blocks per chunk).  A chunk is compressed by the block kernels into the bound-sized slots of one of the three stages
 * (stream A), and its frame records are moved from there straight to their place in d_dst by lz_frame_scan_kernel /
 * lz_frame_gather_kernel (lz_frame_pack.h, stream B).  WHERE that place is only the device knows: the scan starts at a 64-bit cursor
 * in device memory and advances it, so all chunks of a call are enqueued without the host waiting for any of them.  The stages'
 * slots rotate under events: the block kernels of chunk k wait for the gather of chunk k - 3, the scan of chunk k for its block
 * kernels; the gather of chunk k runs beside the block kernels of chunk k + 1.  The host writes the header up front and, once it has
 * read the final cursor (32 bytes, the only wait of the call besides the checksum's), the end mark and the checksum behind it.
 *
 * Capacity.  dstCapacity >= LizardGPU_compressFrameBound is required up front, as by the twin.  One input can still exceed such a
 * buffer: a 1-byte last block is a 10-byte record where the bound counted 5 (lizard_frame_host.c, frame_records).  The twin answers
 * dstMaxSize_tooSmall then, and so does this file: the kernels take a byte limit (dstCapacity minus end mark and checksum), write no
 * record that ends behind it, and raise a flag the host reads with the cursor.
 * Content checksum: XXH32 on the HOST (lizard_unframe_device.c says why).  With a checksum the SOURCE crosses PCIe once, D2H in
 * pieces through two pinned buffers on stream C, hashed by the calling thread while the device compresses. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_common.h"
#include "lizard_xxhash.h"

#ifndef LZC_HASH_PIECE                                       /* (the fake-device tests build with a small odd piece) */
#define LZC_HASH_PIECE    ((size_t)32 << 20)                 /* source bytes per D2H copy of the checksum pass */
#endif

/* the small pinned area of a call (stage 0's h_aux): header, the state the cursor starts from, the state read back, end mark + checksum */
enum { LZC_H_HEADER = 0, LZC_H_INIT = 32, LZC_H_RESULT = 64, LZC_H_TAIL = 96, LZC_H_BYTES = 128 };
/* a stage's device tables (its d_aux): [64: stage 0 keeps the state here][sizes][offsets] */
#define LZC_STATE_BYTES 64u
static size_t c_aux_bytes(size_t P) { return LZC_STATE_BYTES + ((4 * P + 7) & ~(size_t)7) + 8 * (P + 1); }

typedef struct {
    LzCtx* c;
    const uint8_t* src; size_t srcSize; uint8_t* dst; size_t cap;
    size_t blockSize, nb, last, perChunk, nChunks, slot, headerBytes, limit;
    int level, hash;
    uint8_t* pin;
    hipStream_t A, B, C;
    Lizard_XXH32_state_t xxh;
} CJob;

static int c_buffers(CJob* j)
{
    LzCtx* c = j->c;
    const size_t P = j->nb < j->perChunk ? j->nb : j->perChunk;
    size_t s;
    int rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[0].h_aux, &c->stage[0].h_aux_cap, LZC_H_BYTES))) return rc;
    j->pin = c->stage[0].h_aux;
    for (s = 0; s < LZ_STAGES && s < j->nChunks; s++) {
        if ((rc = lzp_ensure_dev(c, (void**)&c->stage[s].d_slots, &c->stage[s].d_slots_cap, P * j->slot))) return rc;
        if ((rc = lzp_ensure_dev(c, (void**)&c->stage[s].d_aux, &c->stage[s].d_aux_cap, c_aux_bytes(P)))) return rc;
    }
    j->A = c->stage[0].stream; j->B = c->stage[1].stream; j->C = c->stage[2].stream;
    return 0;
}

/* header, cursor and every chunk: enqueued, nothing waited for */
static int c_enqueue(CJob* j)
{
    LzCtx* c = j->c;
    const size_t P = j->nb < j->perChunk ? j->nb : j->perChunk;
    uint64_t* const d_state = (uint64_t*)c->stage[0].d_aux;
    size_t k;
    int rc;
    LZ_HIP(hipMemcpyAsync(j->dst, j->pin + LZC_H_HEADER, j->headerBytes, hipMemcpyHostToDevice, j->B));
    if (!j->nb) return 0;
    LZ_HIP(hipMemcpyAsync(d_state, j->pin + LZC_H_INIT, 32, hipMemcpyHostToDevice, j->B));
    for (k = 0; k < j->nChunks; k++) {
        LzStage* s = &c->stage[k % LZ_STAGES];
        const size_t first = k * j->perChunk, q = j->nb - first < j->perChunk ? j->nb - first : j->perChunk;
        const size_t last = first + q == j->nb ? j->last : j->blockSize;
        uint32_t* const d_sizes = (uint32_t*)(s->d_aux + LZC_STATE_BYTES);
        uint64_t* const d_offsets = (uint64_t*)(s->d_aux + LZC_STATE_BYTES + ((4 * P + 7) & ~(size_t)7));
        const uint8_t* const in = j->src + first * j->blockSize;
        if (k >= LZ_STAGES) LZ_HIP(hipStreamWaitEvent(j->A, s->done, 0));      /* the slots and tables are free once chunk k - 3 is gathered */
        if ((rc = lzk_launch(c, in, q, j->blockSize, last, s->d_slots, j->slot, d_sizes, j->level, j->A, s->k0, s->k1, NULL, NULL))) return rc;
        LZ_HIP(hipStreamWaitEvent(j->B, s->k1, 0));
        if ((rc = lzk_frame_pack_launch(in, s->d_slots, j->slot, d_sizes, d_offsets, j->dst, (uint32_t)q, (uint32_t)j->blockSize, (uint32_t)last,
                                        d_state, (uint64_t)j->limit, j->B))) return rc;
        LZ_HIP(hipEventRecord(s->done, j->B));
        c->devFrameCompressStats[2]++;
    }
    LZ_HIP(hipMemcpyAsync(j->pin + LZC_H_RESULT, d_state, 32, hipMemcpyDeviceToHost, j->B));
    LZ_HIP(hipEventRecord(c->stage[0].meta, j->B));
    return 0;
}

/* the content checksum over the source: D2H in pieces through two pinned buffers, the copy of a piece behind the hashing of the one
 * before it, while the chunks run on the other streams */
static int c_hash_source(CJob* j)
{
    LzStage* s = j->c->stage;
    hipEvent_t ev[2];
    const size_t n = j->srcSize, nPieces = (n + LZC_HASH_PIECE - 1) / LZC_HASH_PIECE;
    size_t i;
    int rc;
    if (!j->hash || !n) return 0;
    ev[0] = s[2].meta; ev[1] = s[1].meta;
    for (i = 0; i < 2; i++) if ((rc = lzp_ensure_pinned((void**)&s[i].h_out, &s[i].h_out_cap, n < LZC_HASH_PIECE ? n : LZC_HASH_PIECE))) return rc;
    for (i = 0; i <= nPieces; i++) {
        if (i < nPieces) {
            const size_t o = i * LZC_HASH_PIECE, m = n - o < LZC_HASH_PIECE ? n - o : LZC_HASH_PIECE;
            LZ_HIP(hipMemcpyAsync(s[i & 1].h_out, j->src + o, m, hipMemcpyDeviceToHost, j->C));
            LZ_HIP(hipEventRecord(ev[i & 1], j->C));
            j->c->devFrameCompressStats[3] += m;
        }
        if (i) {
            const size_t o = (i - 1) * LZC_HASH_PIECE, m = n - o < LZC_HASH_PIECE ? n - o : LZC_HASH_PIECE;
            LZ_HIP(hipEventSynchronize(ev[(i - 1) & 1]));
            Lizard_XXH32_update(&j->xxh, s[(i - 1) & 1].h_out, m);
        }
    }
    return 0;
}

static void c_wr32le(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* waits for the cursor, writes end mark and checksum behind it.  *result: the frame's size or dstMaxSize_tooSmall */
static int c_finish(CJob* j, int checksumFlag, size_t frameEnd, size_t* result)
{
    LzCtx* c = j->c;
    uint64_t st[4] = { (uint64_t)j->headerBytes, 0, 0, 0 };
    size_t tail = 4;
    if (j->nb) {
        LZ_HIP(hipEventSynchronize(c->stage[0].meta));
        memcpy(st, j->pin + LZC_H_RESULT, sizeof st);
    }
    if (st[1] || st[0] > (uint64_t)j->limit || j->cap - (size_t)st[0] < frameEnd) { *result = LZ_FRAME_E(dstMaxSize_tooSmall); return 0; }
    c_wr32le(j->pin + LZC_H_TAIL, 0);
    if (checksumFlag == 1) { c_wr32le(j->pin + LZC_H_TAIL + 4, Lizard_XXH32_digest(&j->xxh)); tail = 8; }
    LZ_HIP(hipMemcpyAsync(j->dst + (size_t)st[0], j->pin + LZC_H_TAIL, tail, hipMemcpyHostToDevice, j->B));
    LZ_HIP(hipStreamSynchronize(j->B));
    c->devFrameCompressStats[0] += (unsigned long long)j->nb - st[2];
    c->devFrameCompressStats[1] += st[2];
    *result = (size_t)st[0] + tail;
    return 0;
}

static size_t c_refuse(size_t code)
{
    snprintf(lzk_err(), LZK_ERR_BYTES, "frame refused: %s", LizardF_getErrorName(code));
    return code;
}

size_t LizardGPU_compressFrame_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize,
                                      const LizardGPU_framePrefs_t* preferencesPtr, void* stream)
{
    LizardF_preferences_t prefs;
    CJob j;
    LzGuard g;
    size_t result, frameEnd;
    int rc;
    lzk_err()[0] = 0;
    /* compress_frame, LizardF_compressBegin and LizardF_compressUpdate of lizard_frame_host.c, in their order */
    result = lzgpu_frame_device_plan(&prefs, preferencesPtr, d_dst, dstCapacity, d_src, srcSize);
    if (result == LZ_FRAME_E(GENERIC)) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null pointer)"); return result; }
    if (result) return c_refuse(result);
    memset(&j, 0, sizeof j);
    j.blockSize = lzgpu_frame_block_size((unsigned)prefs.frameInfo.blockSizeID);
    j.level = lzk_clamp_level(prefs.compressionLevel);
    frameEnd = 4 + (size_t)prefs.frameInfo.contentChecksumFlag * 4;

    j.src = (const uint8_t*)d_src; j.srcSize = srcSize; j.dst = (uint8_t*)d_dst; j.cap = dstCapacity;
    j.nb = (srcSize + j.blockSize - 1) / j.blockSize;
    j.last = j.nb ? srcSize - (j.nb - 1) * j.blockSize : 0;
    j.slot = lz_bound_slot(j.blockSize);
    j.limit = dstCapacity - frameEnd;                          /* (the bound counts frameEnd) */
    j.hash = prefs.frameInfo.contentChecksumFlag == 1;
    Lizard_XXH32_reset(&j.xxh, 0);
    lzk_guard_acquire(&g);
    if (g.rc) return LZ_FRAME_E(GENERIC);
    j.c = g.c;
    rc = lzk_ctx_init(g.c);
    if (!rc) {
        j.perChunk = lz_frame_chunk_blocks(g.c, j.blockSize);
        j.nChunks = (j.nb + j.perChunk - 1) / j.perChunk;
        rc = c_buffers(&j);
    }
    if (!rc) {
        uint64_t init[4] = { 0, 0, 0, 0 };
        j.headerBytes = lzgpu_frame_write_header(j.pin + LZC_H_HEADER, &prefs.frameInfo);
        init[0] = (uint64_t)j.headerBytes;
        memcpy(j.pin + LZC_H_INIT, init, sizeof init);
        g.c->hostKernelMs = -1.0f;
        rc = lz_order_after(g.c, (hipStream_t)stream, j.A, j.B, j.C);
    }
    if (!rc) rc = c_enqueue(&j);
    if (!rc) rc = c_hash_source(&j);
    if (!rc) rc = c_finish(&j, (int)prefs.frameInfo.contentChecksumFlag, frameEnd, &result);
    lz_quiesce(g.c);
    lzk_guard_release(&g);
    if (rc) return LZ_FRAME_E(GENERIC);
    if (LizardGPU_frameIsError(result)) return c_refuse(result);
    return result;
}

int LizardGPU_frameCompressDeviceStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devFrameCompressStats));
}
