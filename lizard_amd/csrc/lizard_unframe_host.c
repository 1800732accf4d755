/* lizard_unframe_host.c — LizardGPU_decompressFrame: the host side of whole-frame decompression on the GPU (include/lizard_amd.h
 * Part 3b).  Plain C on the HIP runtime's C API and the shim of lizard_gpu_ctx.h, like lizard_pipeline_host.c, whose staging
 * helpers it shares; the kernel is lz_unframe_kernel (unframe_kernels.h), the frame walk LizardGPU_frameIndex (lizard_frame_host.c). */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_common.h"
#define ensure_dev     lzp_ensure_dev
#define ensure_pinned  lzp_ensure_pinned
#define par_memcpy     lzp_par_memcpy
#define is_pinned_host lzp_is_pinned_host
#define chunk_bytes    lzp_chunk_bytes

/* ================================================= frame decoding =================================================
 * LizardGPU_decompressFrame: one frame in host memory -> its decoded bytes.  The host walks the header and the chain of block
 * records (LizardGPU_frameIndex, lizard_frame_host.c) and cuts the records into chunks of at most LIZARDGPU_CHUNK_MB of output
 * slots (one slot = the frame's maximum block size per record; a record larger than a chunk is a chunk of its own).  Per chunk,
 * on its stage's stream: the chunk's span of the frame -> pinned staging (skipped when src is pinned) -> H2D, with the record
 * table -> lz_unframe_kernel (one wave per record) -> D2H of the per-record results.  Up to LZ_STAGES chunks are in flight.
 * The calling thread finishes the chunks IN ORDER: when every slot but the last is full the slots are the decoded bytes and come
 * back with one D2H; otherwise the valid bytes are packed on the device first (lz_pack.h).  Good blocks are copied from staging to
 * dst; a block of a linked frame that reaches into its history (LZD_NEED_HISTORY) is decoded by the host decoder right behind the
 * bytes that are final by then; the content checksum is fed in the same pass.  The copy of the next chunk is requested before
 * the current one is finished, so PCIe, the kernels and the host copies of different chunks overlap. */
#include "lizard_xxhash.h"

#define LZU_NEED_HISTORY 0xFFFFFFFEu
#define LZU_DICT         ((size_t)1 << 24)                  /* LIZARD_DICT_SIZE: no offset reaches further back */
/* A frame whose blocks lean on their history gains nothing from the device: each such block is decoded twice.  When at least this
 * share of a chunk's records came back as LZD_NEED_HISTORY the rest of the frame goes to the host decoder directly.  The two
 * populations are far apart — measured with the compiled reference on 2 MiB of datagen P50 and text, levels 10 / 17 / 30 / 41,
 * block size ids 1 and 2: every block but the first of a reference-made linked frame needs its history (15 of 16, 7 of 8), no
 * block of a frame this library writes does (Lizard_compress_continue is history-free) — so any value well inside (0, 1) tells
 * them apart; one half is the midpoint.  The first chunk of a linked frame is kept to LZU_PROBE_RECORDS records so that what is
 * wasted on the wrong guess is small.  Correctness does not depend on it: LIZARDGPU_UNFRAME_HOST_SHARE overrides it (0 = the first
 * block that needs history ends the device part, above 1 = never). */
#define LZU_HOST_SHARE     0.5
#define LZU_PROBE_RECORDS  64

typedef struct { size_t first, n, spanOff, spanBytes, outBytes; int packed; } UChunk;
typedef struct {
    LzCtx* c;
    const uint8_t* src; uint8_t* dst; size_t cap;
    const uint64_t* off; const uint32_t* words; size_t nRecords;
    size_t maxBlock; int linked, checksum, srcPinned, giveUp;
    unsigned long long contentSize;
    double hostShare;
    size_t pos, hashed;                                      /* dst[0..pos) is final; dst[0..hashed) has been fed to the checksum */
    uint8_t* tmp;                                            /* one block, for a host-decoded block that may not fit what is left of dst */
    Lizard_XXH32_state_t xxh;
} UJob;

static size_t uf_words_bytes(size_t n) { return 4 * ((n + 1) & ~(size_t)1); }

static int uf_issue(UJob* j, LzStage* s, UChunk* ch, hipEvent_t prevUp)
{
    LzCtx* c = j->c;
    const size_t n = ch->n, wb = uf_words_bytes(n);
    const size_t dAux = 8 * n + wb + 8 * (n + 1) + 8 * n, hAux = 8 * n + wb + 4 * n;
    const uint8_t* from = j->src + ch->spanOff;
    uint64_t* rel; uint32_t* w;
    size_t i;
    int rc;
    if ((rc = ensure_dev(c, (void**)&s->d_in, &s->d_in_cap, ch->spanBytes + 64))) return rc;
    if ((rc = ensure_dev(c, (void**)&s->d_slots, &s->d_slots_cap, n * j->maxBlock))) return rc;
    if ((rc = ensure_pinned((void**)&s->h_out, &s->h_out_cap, n * j->maxBlock + 64))) return rc;
    if (s->d_aux_cap < dAux) {
        if (s->d_aux) { (void)hipFree(s->d_aux); s->d_aux = NULL; s->d_aux_cap = 0; }
        LZ_HIP(hipMalloc((void**)&s->d_aux, dAux));
        s->d_aux_cap = dAux;
    }
    if ((rc = ensure_pinned((void**)&s->h_aux, &s->h_aux_cap, hAux))) return rc;
    rel = (uint64_t*)s->h_aux; w = (uint32_t*)(s->h_aux + 8 * n);
    for (i = 0; i < n; i++) { rel[i] = j->off[ch->first + i] - ch->spanOff; w[i] = j->words[ch->first + i]; }
    if (!j->srcPinned) {
        if ((rc = ensure_pinned((void**)&s->h_in, &s->h_in_cap, ch->spanBytes))) return rc;
        par_memcpy(s->h_in, from, ch->spanBytes);
        from = s->h_in;
    }
    if (prevUp) LZ_HIP(hipStreamWaitEvent(s->stream, prevUp, 0));
    LZ_HIP(hipMemcpyAsync(s->d_in, from, ch->spanBytes, hipMemcpyHostToDevice, s->stream));
    LZ_HIP(hipMemcpyAsync(s->d_aux, s->h_aux, 8 * n + wb, hipMemcpyHostToDevice, s->stream));
    LZ_HIP(hipEventRecord(s->up, s->stream));
    {
        uint32_t* dOut = (uint32_t*)(s->d_aux + 8 * n + wb + 8 * (n + 1));
        if ((rc = lzk_launch_unframe(c, s->d_in, (const uint64_t*)s->d_aux, (const uint32_t*)(s->d_aux + 8 * n), n, s->d_slots, j->maxBlock,
                                     dOut, dOut + n, s->stream))) return rc;
        LZ_HIP(hipMemcpyAsync(s->h_aux + 8 * n + wb, dOut, 4 * n, hipMemcpyDeviceToHost, s->stream));
    }
    LZ_HIP(hipEventRecord(s->meta, s->stream));
    return 0;
}

/* results known -> request the decoded bytes: the slots as they are, or packed first when one in the middle is not full */
static int uf_fetch(UJob* j, LzStage* s, UChunk* ch)
{
    const size_t n = ch->n, wb = uf_words_bytes(n);
    const uint32_t* out = (const uint32_t*)(s->h_aux + 8 * n + wb);
    size_t i, sum = 0;
    int allFull = 1, rc;
    LZ_HIP(hipEventSynchronize(s->meta));
    for (i = 0; i < n; i++) {
        const size_t valid = out[i] >= LZU_NEED_HISTORY ? 0 : out[i];
        if (i + 1 < n && valid != j->maxBlock) allFull = 0;
        sum += valid;
    }
    ch->packed = !allFull; ch->outBytes = sum;
    if (allFull) {
        if (sum) LZ_HIP(hipMemcpyAsync(s->h_out, s->d_slots, sum, hipMemcpyDeviceToHost, s->stream));
    } else {
        uint32_t* dOut = (uint32_t*)(s->d_aux + 8 * n + wb + 8 * (n + 1));
        if ((rc = ensure_dev(j->c, (void**)&s->d_packed, &s->d_packed_cap, sum + 64))) return rc;
        lzk_pack_launch(NULL, s->d_slots, j->maxBlock, dOut + n, (uint64_t*)(s->d_aux + 8 * n + wb), s->d_packed, (uint32_t)n, 0, 0, LZK_PACK_PAYLOAD, s->stream);
        LZ_HIP(hipGetLastError());
        if (sum) LZ_HIP(hipMemcpyAsync(s->h_out, s->d_packed, sum, hipMemcpyDeviceToHost, s->stream));
        j->c->unframeStats[4]++;
    }
    LZ_HIP(hipEventRecord(s->done, s->stream));
    return 0;
}

/* the caller's buffer cannot take `n` more bytes: a header content size it does hold says the frame, not the buffer, is wrong */
static size_t uf_no_room(const UJob* j) { return j->contentSize && j->cap >= j->contentSize ? LZ_FRAME_E(frameSize_wrong) : LZ_FRAME_E(dstMaxSize_tooSmall); }

static void uf_hash_to(UJob* j) { if (j->checksum && j->pos > j->hashed) Lizard_XXH32_update(&j->xxh, j->dst + j->hashed, j->pos - j->hashed); j->hashed = j->pos; }

/* one compressed record on the host decoder, behind the final bytes dst[0..pos).  0 or a frame error code. */
static size_t uf_host_block(UJob* j, size_t rec)
{
    const size_t size = j->words[rec] & 0x7FFFFFFFu, room = j->cap - j->pos;
    const size_t d = j->linked ? (j->pos < LZU_DICT ? j->pos : LZU_DICT) : 0;
    const char* payload = (const char*)j->src + j->off[rec];
    int r;
    if (room >= j->maxBlock) r = Lizard_decompress_safe_usingDict(payload, (char*)j->dst + j->pos, (int)size, (int)j->maxBlock, (const char*)j->dst + j->pos - d, (int)d);
    else {
        if (!j->tmp && !(j->tmp = (uint8_t*)malloc(j->maxBlock))) return LZ_FRAME_E(allocation_failed);
        r = Lizard_decompress_safe_usingDict(payload, (char*)j->tmp, (int)size, (int)j->maxBlock, (const char*)j->dst + j->pos - d, (int)d);
        if (r >= 0 && (size_t)r > room) return uf_no_room(j);
        if (r > 0) memcpy(j->dst + j->pos, j->tmp, (size_t)r);
    }
    if (r < 0) return j->linked ? LZ_FRAME_E(decompressionFailed) : LZ_FRAME_E(GENERIC);
    j->pos += (size_t)r;
    return 0;
}

static size_t uf_drain(UJob* j, LzStage* s, UChunk* ch)
{
    const size_t n = ch->n, wb = uf_words_bytes(n);
    const uint32_t* out = (const uint32_t*)(s->h_aux + 8 * n + wb);
    const uint8_t* p = s->h_out;                             /* staging: next good block */
    const uint8_t* runSrc = p; size_t runLen = 0;            /* good blocks are contiguous in staging and in dst: copied run by run */
    size_t i, needHist = 0;
    if (hipEventSynchronize(s->done) != hipSuccess) { snprintf(lzk_err(), LZK_ERR_BYTES, "hipEventSynchronize failed: %s", hipGetErrorString(hipGetLastError())); return LZ_FRAME_E(GENERIC); }
    for (i = 0; i < n; i++) {
        const uint32_t r = out[i];
        const int raw = (j->words[ch->first + i] >> 31) != 0;
        if (r >= LZU_NEED_HISTORY) {
            size_t e;
            if (r != LZU_NEED_HISTORY || !j->linked) return j->linked ? LZ_FRAME_E(decompressionFailed) : LZ_FRAME_E(GENERIC);
            if (runLen) { par_memcpy(j->dst + j->pos - runLen, runSrc, runLen); runLen = 0; }
            uf_hash_to(j);
            if ((e = uf_host_block(j, ch->first + i))) return e;
            needHist++; j->c->unframeStats[2]++;
            runSrc = p;
            continue;
        }
        if (r > j->cap - j->pos) return uf_no_room(j);
        if (!runLen) runSrc = p;
        runLen += r; j->pos += r; p += ch->packed ? r : j->maxBlock;
        if (!ch->packed && r != j->maxBlock && i + 1 < n) return LZ_FRAME_E(GENERIC);          /* (uf_fetch packs such a chunk) */
        j->c->unframeStats[raw ? 1 : 0]++;
    }
    if (runLen) par_memcpy(j->dst + j->pos - runLen, runSrc, runLen);
    uf_hash_to(j);
    if (j->linked && needHist && (double)needHist >= j->hostShare * (double)n) j->giveUp = 1;
    return 0;
}

static size_t uf_run(UJob* j)
{
    LzCtx* c = j->c;
    UChunk ch[LZ_STAGES];
    size_t perChunk = chunk_bytes(c) / j->maxBlock, issued = 0, fetched = 0, drained = 0, nextRec = 0, e;
    int rc;
    if (perChunk == 0) perChunk = 1;
    if ((rc = lzk_ctx_init(c))) return LZ_FRAME_E(GENERIC);
    c->hostKernelMs = -1.0f;
    while (drained < issued || (nextRec < j->nRecords && !j->giveUp)) {
        while (issued - drained < LZ_STAGES && nextRec < j->nRecords && !j->giveUp) {
            UChunk* k = &ch[issued % LZ_STAGES];
            size_t n = j->nRecords - nextRec < perChunk ? j->nRecords - nextRec : perChunk, last;
            if (j->linked && issued == 0 && n > LZU_PROBE_RECORDS) n = LZU_PROBE_RECORDS;
            last = nextRec + n - 1;
            k->first = nextRec; k->n = n; k->spanOff = (size_t)j->off[nextRec];
            k->spanBytes = (size_t)j->off[last] + (j->words[last] & 0x7FFFFFFFu) - k->spanOff;
            if (uf_issue(j, &c->stage[issued % LZ_STAGES], k, issued ? c->stage[(issued - 1) % LZ_STAGES].up : NULL)) return LZ_FRAME_E(GENERIC);
            issued++; nextRec += n;
        }
        for (; fetched < issued && fetched < drained + 2; fetched++)
            if (uf_fetch(j, &c->stage[fetched % LZ_STAGES], &ch[fetched % LZ_STAGES])) return LZ_FRAME_E(GENERIC);
        if ((e = uf_drain(j, &c->stage[drained % LZ_STAGES], &ch[drained % LZ_STAGES]))) return e;
        drained++;
        if (j->giveUp) { nextRec = ch[(drained - 1) % LZ_STAGES].first + ch[(drained - 1) % LZ_STAGES].n; break; }
    }
    if (j->giveUp && nextRec < j->nRecords) {                /* the rest on the host decoder; what is still in flight is dropped by the caller's drain */
        size_t i;
        c->unframeStats[3]++;
        for (i = nextRec; i < j->nRecords; i++) {
            const size_t size = j->words[i] & 0x7FFFFFFFu;
            if (j->words[i] >> 31) {
                if (size > j->cap - j->pos) return uf_no_room(j);
                memcpy(j->dst + j->pos, j->src + j->off[i], size);
                j->pos += size;
            } else if ((e = uf_host_block(j, i))) return e;
        }
        uf_hash_to(j);
    }
    return 0;
}

size_t LizardGPU_decompressFrame(void* dst, size_t dstCapacity, const void* src, size_t srcSize, size_t* srcConsumedPtr)
{
    LizardGPU_frameInfo_t info;
    UJob j;
    LzGuard g;
    uint64_t* off = NULL; uint32_t* words = NULL;
    size_t n = 0, frameBytes = 0, result;
    int rc;
    if (srcConsumedPtr) *srcConsumedPtr = 0;
    lzk_err()[0] = 0;
    if ((!dst && dstCapacity) || (!src && srcSize)) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null pointer)"); return LZ_FRAME_E(GENERIC); }
    if ((rc = LizardGPU_frameIndex(src, srcSize, &info, NULL, NULL, 0, &n, &frameBytes))) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "frame refused: %s", LizardF_getErrorName((size_t)(long)rc));
        return (size_t)(long)rc;
    }
    memset(&j, 0, sizeof j);
    j.src = (const uint8_t*)src; j.dst = (uint8_t*)dst; j.cap = dstCapacity;
    j.checksum = info.contentChecksumFlag != 0; j.linked = info.blockMode == LizardF_blockLinked; j.contentSize = info.contentSize;
    result = 0;
    if (info.frameType != LizardF_skippableFrame) {
        Lizard_XXH32_reset(&j.xxh, 0);
        if (n) {
            const char* e = getenv("LIZARDGPU_UNFRAME_HOST_SHARE");
            off = (uint64_t*)malloc(n * sizeof *off); words = (uint32_t*)malloc(n * sizeof *words);
            if (!off || !words) { free(off); free(words); snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); return LZ_FRAME_E(allocation_failed); }
            (void)LizardGPU_frameIndex(src, srcSize, &info, off, words, n, &n, &frameBytes);
            j.off = off; j.words = words; j.nRecords = n;
            j.maxBlock = lzgpu_frame_block_size((unsigned)info.blockSizeID);
            j.hostShare = e && *e ? strtod(e, NULL) : LZU_HOST_SHARE;
            lzk_guard_acquire(&g);
            if (g.rc) result = LZ_FRAME_E(GENERIC);
            else {
                j.c = g.c;
                j.srcPinned = is_pinned_host(src);
                result = uf_run(&j);
                lz_quiesce(g.c);                               /* copies of chunks that were not finished (an error, or the hand-over to the host decoder) may still be in flight */
                lzk_guard_release(&g);
            }
            free(j.tmp); free(off); free(words);
        }
        if (!result && j.contentSize && (unsigned long long)j.pos != j.contentSize) result = LZ_FRAME_E(frameSize_wrong);
        if (!result && j.checksum) {
            const uint8_t* q = (const uint8_t*)src + frameBytes - 4;
            const uint32_t stored = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            if (stored != Lizard_XXH32_digest(&j.xxh)) result = LZ_FRAME_E(contentChecksum_invalid);
        }
        if (result) {
            if (!lzk_err()[0]) snprintf(lzk_err(), LZK_ERR_BYTES, "frame refused: %s", LizardF_getErrorName(result));
            return result;
        }
    }
    if (srcConsumedPtr) *srcConsumedPtr = frameBytes;
    return j.pos;
}

int LizardGPU_frameDecodeStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, unframeStats));    /* (the first four of five: LizardGPU_frameDecodePackedChunks has the fifth) */
}

unsigned long long LizardGPU_frameDecodePackedChunks(void)
{
    LzCtx* c = lzk_ctx_peek();
    unsigned long long v;
    if (!c) return 0;
    pthread_mutex_lock(&c->mu);
    v = c->unframeStats[4];
    pthread_mutex_unlock(&c->mu);
    return v;
}
