/* lizard_unframe_device.c — LizardGPU_decompressFrame_device / LizardGPU_frameIndex_device: whole-frame decompression when the
 * frame already lies in device memory and the decoded bytes are wanted there (include/lizard_amd.h Part 3b).  Plain C on the HIP
 * runtime's C API and the shim of lizard_gpu_ctx.h, like lizard_unframe_host.c, whose result it reproduces for every input.
 *
 * Nothing but a few hundred bytes per segment crosses PCIe.  The frame is walked ON THE DEVICE (lz_unframe_walk_kernel,
 * unframe_walk.h) in segments of LZ_WALK_RECORDS records (LIZARDGPU_WALK_RECORDS overrides), on a stream of its own; the host
 * fetches the small result record of a segment, starts the walk of the next one, and decodes the segment it has on another
 * stream meanwhile, so the dependent loads of the chain hide behind the decode.  A segment is decoded IN PLACE
 * (lz_unframe_inplace_kernel): record i goes to d_dst + pos + i * maxBlock, where it belongs when every earlier record fills its
 * block — true of every frame but flushed ones — so the decoded frame is never copied.  pos is exact at the start of every segment:
 * the host reads the per-record results (4 bytes each) before it goes on.  The records of a segment behind the first short one, a
 * record whose slot would start at or behind dstCapacity, and a record that failed in a short last slot are decoded once more into
 * the context's staging slots, LIZARDGPU_CHUNK_MB at a time, and moved into place device to device by lz_scan_kernel /
 * lz_gather_kernel (lz_pack.h) — never packed in place over overlapping ranges.
 *
 * Order of the answers = the host twin's: it finishes its walk before it decodes, so a refusal of the chain outranks a corrupt
 * block or a buffer that is too small; after a decode-stage error this file decodes nothing more but walks on to the end mark.
 * A block that needs its history (LZD_NEED_HISTORY: the reference's linked frames, never this library's) ends the device part:
 * the frame is copied to pinned host memory, decoded by LizardGPU_decompressFrame and the result copied into d_dst.
 * The content checksum (XXH32: four serial multiply-rotate chains over the whole stream) is computed on the HOST: unless
 * LIZARDGPU_FRAME_SKIP_CHECKSUM is given the decoded bytes cross PCIe once, in pieces through pinned staging, and are hashed by
 * the calling thread: the bytes of a segment while the NEXT segment decodes, those of the last (or only) segment after it.  The
 * call is bounded by the host's hashing rate either way. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_common.h"
#include "lizard_xxhash.h"

/* Records per walk segment.  A decode launch has one wave per record and lasts as long as its slowest wave, and the launches of
 * successive segments share the context's arena, so they run one after the other.  Measured with 1 024 records per segment
 * (profiles/frame_decode_device.json; 1 GiB frame, 4 096 records of 256 KiB, level 10): the call takes
 * 17.0 ms in 5 segments where the block decoder takes 4.2 ms for all 4 096 blocks in one launch, and the walk alone 1.1 ms
 * (0.27 us per record).  The default below follows from that by reasoning and has NOT been measured yet: as many records as the
 * device has decoding waves (256 CUs x 16), so that one launch can fill it; a larger segment only delays the first decode behind a
 * longer walk. */
#define LZ_WALK_RECORDS   4096
#define LZV_NEED_HISTORY  0xFFFFFFFEu
#ifndef LZV_HASH_PIECE                                       /* (the fake-device tests build with a small odd piece) */
#define LZV_HASH_PIECE    ((size_t)32 << 20)                 /* decoded bytes per D2H copy of the checksum pass */
#endif

static size_t walk_records(void)
{
    const char* e = getenv("LIZARDGPU_WALK_RECORDS");
    const unsigned long v = e && *e ? strtoul(e, NULL, 10) : 0;
    return v >= 1 && v <= (1ul << 20) ? (size_t)v : LZ_WALK_RECORDS;
}

/* the device tables of one segment: offsets, scan output of the gather path, words, results, valid bytes, result record */
typedef struct { uint64_t* offs; uint64_t* scan; uint32_t* words; uint32_t* out; uint32_t* pack; LzWalkResult* res; } VSet;
static size_t vset_bytes(size_t B) { return ((28 * B + 8 + 63) & ~(size_t)63) + 128; }
static size_t hset_bytes(size_t B) { return 128 + ((4 * B + 63) & ~(size_t)63); }

typedef struct {
    LzCtx* c;
    const uint8_t* src; size_t srcSize; uint8_t* dst; size_t cap; int hash;
    size_t B, maxBlock; int linked, checksum;
    unsigned long long contentSize;
    size_t pos, hashed, totalRecords, frameBytes, headerBytes;
    size_t pendErr; int needHost;
    VSet d[2]; LzWalkResult* hres[2]; uint32_t* hout[2];
    hipStream_t W, D, C;
    Lizard_XXH32_state_t xxh;
} VJob;

static int v_buffers(VJob* j)
{
    LzCtx* c = j->c;
    const size_t B = j->B;
    int rc, k;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, 2 * vset_bytes(B)))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&c->stage[0].h_aux, &c->stage[0].h_aux_cap, 2 * hset_bytes(B)))) return rc;
    for (k = 0; k < 2; k++) {
        uint8_t* p = c->dfTab + (size_t)k * vset_bytes(B);
        uint8_t* h = c->stage[0].h_aux + (size_t)k * hset_bytes(B);
        j->d[k].offs = (uint64_t*)p; j->d[k].scan = (uint64_t*)(p + 8 * B); j->d[k].words = (uint32_t*)(p + 16 * B + 8);
        j->d[k].out = j->d[k].words + B; j->d[k].pack = j->d[k].out + B;
        j->d[k].res = (LzWalkResult*)(p + vset_bytes(B) - 128);
        j->hres[k] = (LzWalkResult*)h; j->hout[k] = (uint32_t*)(h + 128);
    }
    j->W = c->stage[0].stream; j->D = c->stage[1].stream; j->C = c->stage[2].stream;
    return 0;
}

static hipEvent_t walk_event(VJob* j, int set) { return set ? j->c->stage[0].done : j->c->stage[0].meta; }

static int v_issue_walk(VJob* j, int set, size_t startPos, size_t budget, size_t tableCap, uint64_t* offs, uint32_t* words)
{
    int rc;
    if ((rc = lzk_launch_walk(j->c, j->src, j->srcSize, startPos, budget, tableCap, offs, words, j->d[set].res, j->W))) return rc;
    LZ_HIP(hipMemcpyAsync(j->hres[set], j->d[set].res, sizeof(LzWalkResult), hipMemcpyDeviceToHost, j->W));
    LZ_HIP(hipEventRecord(walk_event(j, set), j->W));
    j->c->devFrameStats[3]++;
    return 0;
}

/* the content checksum over dst[hashed..upto), final bytes: D2H in pieces through two pinned buffers, the copy of a piece behind
 * the hashing of the one before it.  The calling thread hashes: called while a segment decodes it covers the segments before that
 * one, so a frame of a single segment (up to LZ_WALK_RECORDS records: 1 GiB at 256 KiB blocks) is hashed after its decode with
 * nothing to overlap, and the last segment of any frame is. */
static int v_hash_to(VJob* j, size_t upto)
{
    LzStage* s = j->c->stage;
    hipEvent_t ev[2];
    size_t at = j->hashed, i, nPieces;
    int rc;
    if (!j->hash || upto <= at) return 0;
    ev[0] = s[2].meta; ev[1] = s[2].done;
    nPieces = (upto - at + LZV_HASH_PIECE - 1) / LZV_HASH_PIECE;
    for (i = 0; i < 2; i++) if ((rc = lzp_ensure_pinned((void**)&s[i].h_out, &s[i].h_out_cap, upto - at < LZV_HASH_PIECE ? upto - at : LZV_HASH_PIECE))) return rc;
    for (i = 0; i <= nPieces; i++) {
        if (i < nPieces) {
            const size_t o = at + i * LZV_HASH_PIECE, n = upto - o < LZV_HASH_PIECE ? upto - o : LZV_HASH_PIECE;
            LZ_HIP(hipMemcpyAsync(s[i & 1].h_out, j->dst + o, n, hipMemcpyDeviceToHost, j->C));
            LZ_HIP(hipEventRecord(ev[i & 1], j->C));
        }
        if (i) {
            const size_t o = at + (i - 1) * LZV_HASH_PIECE, n = upto - o < LZV_HASH_PIECE ? upto - o : LZV_HASH_PIECE;
            LZ_HIP(hipEventSynchronize(ev[(i - 1) & 1]));
            Lizard_XXH32_update(&j->xxh, s[(i - 1) & 1].h_out, n);
        }
    }
    j->hashed = upto;
    return 0;
}

/* the caller's buffer cannot take more bytes: a header content size it does hold says the frame, not the buffer, is wrong */
static size_t v_no_room(const VJob* j) { return j->contentSize && j->cap >= j->contentSize ? LZ_FRAME_E(frameSize_wrong) : LZ_FRAME_E(dstMaxSize_tooSmall); }

/* The n records of the segment in table set `set`, in order behind dst[0..pos).  0, or -LIZARDGPU_ERR_* for a failure of the
 * machinery; what the FRAME has to say goes to j->pendErr / j->needHost. */
static int v_decode_segment(VJob* j, int set, size_t n)
{
    LzCtx* c = j->c;
    const VSet* t = &j->d[set];
    uint32_t* out = j->hout[set];
    hipEvent_t ev = c->stage[1].meta;
    const size_t base = j->pos, final = j->pos;
    size_t m = 0, accepted = 0, i, perChunk = lzp_chunk_bytes(c) / j->maxBlock;
    int rc, gathered = 0;
    if (perChunk == 0) perChunk = 1;
    if (base < j->cap) {
        m = (j->cap - base + j->maxBlock - 1) / j->maxBlock;
        if (m > n) m = n;
    }
    if (m) {
        if ((rc = lzk_launch_unframe_inplace(c, j->src, t->offs, t->words, m, j->dst + base, j->maxBlock, j->cap - base, t->out, t->pack, j->D))) return rc;
        LZ_HIP(hipMemcpyAsync(out, t->out, 4 * m, hipMemcpyDeviceToHost, j->D));
        LZ_HIP(hipEventRecord(ev, j->D));
    }
    if ((rc = v_hash_to(j, final))) return rc;                /* the bytes of the segments before this one, while this one decodes */
    if (m) {
        LZ_HIP(hipEventSynchronize(ev));
        for (i = 0; i < m; i++) {
            if (out[i] >= LZV_NEED_HISTORY) break;
            accepted++; j->pos += out[i];
            if (out[i] != j->maxBlock) break;                 /* what follows a short record sits in the wrong place */
        }
        c->devFrameStats[0] += accepted;
    }
    for (i = accepted; i < n; ) {
        const size_t q = n - i < perChunk ? n - i : perChunk;
        size_t k, sum = 0;
        if ((rc = lzp_ensure_dev(c, (void**)&c->stage[0].d_slots, &c->stage[0].d_slots_cap, q * j->maxBlock))) return rc;
        if ((rc = lzk_launch_unframe(c, j->src, t->offs + i, t->words + i, q, c->stage[0].d_slots, j->maxBlock, t->out + i, t->pack + i, j->D))) return rc;
        LZ_HIP(hipMemcpyAsync(out + i, t->out + i, 4 * q, hipMemcpyDeviceToHost, j->D));
        LZ_HIP(hipEventRecord(ev, j->D));
        LZ_HIP(hipEventSynchronize(ev));
        for (k = 0; k < q; k++) {
            const uint32_t r = out[i + k];
            if (r >= LZV_NEED_HISTORY) {
                if (r == LZV_NEED_HISTORY && j->linked) j->needHost = 1;
                else j->pendErr = j->linked ? LZ_FRAME_E(decompressionFailed) : LZ_FRAME_E(GENERIC);
                return 0;
            }
            if (r > j->cap - j->pos - sum) { j->pendErr = v_no_room(j); return 0; }
            sum += r;
        }
        lzk_pack_launch(NULL, c->stage[0].d_slots, j->maxBlock, t->pack + i, t->scan, j->dst + j->pos, (uint32_t)q, 0, 0, LZK_PACK_PAYLOAD, j->D);
        LZ_HIP(hipGetLastError());
        gathered = 1;
        j->pos += sum; i += q;
        c->devFrameStats[1] += q;
    }
    if (gathered) LZ_HIP(hipStreamSynchronize(j->D));          /* the checksum pass reads these bytes on another stream */
    return 0;
}

/* walk + decode of a normal frame whose first segment is in set 0.  0 or -LIZARDGPU_ERR_*; *chainErr: the walk's refusal. */
static int v_run(VJob* j, unsigned* chainErr)
{
    size_t k;
    int rc;
    for (k = 0;; k++) {
        const int set = (int)(k & 1);
        LzWalkResult r;
        LZ_HIP(hipEventSynchronize(walk_event(j, set)));
        r = *j->hres[set];
        if (r.status) { *chainErr = r.status; return 0; }
        if (!r.done && (rc = v_issue_walk(j, set ^ 1, (size_t)r.nextPos, j->B, j->B, j->d[set ^ 1].offs, j->d[set ^ 1].words))) return rc;
        j->totalRecords += (size_t)r.nRecords;
        if (r.nRecords && !j->pendErr && !j->needHost && (rc = v_decode_segment(j, set, (size_t)r.nRecords))) return rc;
        if (r.done) { j->frameBytes = (size_t)r.frameBytes; return 0; }
    }
}

/* A linked frame with a block that needs its history: the host twin decodes it from a pinned copy, the result goes back. */
static size_t v_finish_on_host(const VJob* j, unsigned flags, size_t* consumed)
{
    uint8_t* hsrc = NULL; uint8_t* hdst = NULL;
    size_t hcap = j->totalRecords * j->maxBlock, used = 0, r, srcBytes = j->frameBytes;
    if (hcap > j->cap) hcap = j->cap;
    if (hipHostMalloc((void**)&hsrc, j->frameBytes, hipHostMallocDefault) != hipSuccess
        || hipHostMalloc((void**)&hdst, hcap ? hcap : 1, hipHostMallocDefault) != hipSuccess
        || hipMemcpy(hsrc, j->src, j->frameBytes, hipMemcpyDeviceToHost) != hipSuccess) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "pinned copy of a linked frame failed: %s", hipGetErrorString(hipGetLastError()));
        if (hsrc) (void)hipHostFree(hsrc);
        if (hdst) (void)hipHostFree(hdst);
        return LZ_FRAME_E(GENERIC);
    }
    if ((flags & LIZARDGPU_FRAME_SKIP_CHECKSUM) && j->checksum) {
        /* the twin always verifies: the copy becomes the same frame without a content checksum (flag cleared, header checksum
         * redone); the 4 bytes behind its end mark are then not part of it */
        const size_t h = j->headerBytes;
        hsrc[4] &= (uint8_t)~4u;
        hsrc[h - 1] = (uint8_t)(Lizard_XXH32(hsrc + 4, h - 5, 0) >> 8);
        srcBytes -= 4;
    }
    r = LizardGPU_decompressFrame(hdst, hcap, hsrc, srcBytes, &used);
    if (!LizardGPU_frameIsError(r)) {
        if (r && hipMemcpy(j->dst, hdst, r, hipMemcpyHostToDevice) != hipSuccess) {
            snprintf(lzk_err(), LZK_ERR_BYTES, "copy of the host-decoded frame failed: %s", hipGetErrorString(hipGetLastError()));
            r = LZ_FRAME_E(GENERIC);
        } else *consumed = j->frameBytes;
    }
    (void)hipHostFree(hsrc); (void)hipHostFree(hdst);
    return r;
}

size_t LizardGPU_decompressFrame_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr,
                                        unsigned flags, void* stream)
{
    VJob j;
    LzGuard g;
    LzWalkResult first;
    unsigned chainErr = 0;
    size_t result = 0, consumed = 0;
    int rc;
    if (srcConsumedPtr) *srcConsumedPtr = 0;
    lzk_err()[0] = 0;
    if ((!d_dst && dstCapacity) || (!d_src && srcSize)) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null pointer)"); return LZ_FRAME_E(GENERIC); }
    memset(&j, 0, sizeof j);
    memset(&first, 0, sizeof first);
    j.src = (const uint8_t*)d_src; j.srcSize = srcSize; j.dst = (uint8_t*)d_dst; j.cap = dstCapacity; j.B = walk_records();
    lzk_guard_acquire(&g);
    if (g.rc) return LZ_FRAME_E(GENERIC);
    j.c = g.c;
    rc = lzk_ctx_init(g.c);
    if (!rc) rc = v_buffers(&j);
    if (!rc) rc = lz_order_after(g.c, (hipStream_t)stream, j.W, j.D, j.C);
    if (!rc) rc = v_issue_walk(&j, 0, 0, j.B, j.B, j.d[0].offs, j.d[0].words);
    if (!rc && hipEventSynchronize(walk_event(&j, 0)) != hipSuccess) { snprintf(lzk_err(), LZK_ERR_BYTES, "the frame walk failed: %s", hipGetErrorString(hipGetLastError())); rc = -LIZARDGPU_ERR_HIP; }
    if (!rc) {
        first = *j.hres[0];
        if (first.status) chainErr = first.status;
        else if (first.frameType) { consumed = (size_t)first.frameBytes; }
        else {
            j.maxBlock = lzgpu_frame_block_size(first.blockSizeID); j.headerBytes = first.headerBytes;
            j.linked = first.blockMode == 0; j.checksum = first.checksumFlag != 0; j.contentSize = first.contentSize;
            j.hash = j.checksum && !(flags & LIZARDGPU_FRAME_SKIP_CHECKSUM);
            Lizard_XXH32_reset(&j.xxh, 0);
            g.c->hostKernelMs = -1.0f;
            rc = v_run(&j, &chainErr);
            if (!rc && !chainErr && !j.pendErr && !j.needHost) {
                if (hipStreamSynchronize(j.D) != hipSuccess) { snprintf(lzk_err(), LZK_ERR_BYTES, "the frame decode failed: %s", hipGetErrorString(hipGetLastError())); rc = -LIZARDGPU_ERR_HIP; }
                else if (j.contentSize && (unsigned long long)j.pos != j.contentSize) j.pendErr = LZ_FRAME_E(frameSize_wrong);
                else if (j.hash) {
                    uint8_t* q = (uint8_t*)j.hres[0] + sizeof(LzWalkResult);   /* pinned: the head of a host set has room behind the result record */
                    rc = v_hash_to(&j, j.pos);
                    if (!rc && hipMemcpyAsync(q, j.src + j.frameBytes - 4, 4, hipMemcpyDeviceToHost, j.C) == hipSuccess && hipStreamSynchronize(j.C) == hipSuccess) {
                        const uint32_t stored = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
                        if (stored != Lizard_XXH32_digest(&j.xxh)) j.pendErr = LZ_FRAME_E(contentChecksum_invalid);
                    } else if (!rc) { snprintf(lzk_err(), LZK_ERR_BYTES, "reading the stored checksum failed: %s", hipGetErrorString(hipGetLastError())); rc = -LIZARDGPU_ERR_HIP; }
                }
                consumed = j.frameBytes;
            }
            if (j.needHost && !chainErr && !rc) g.c->devFrameStats[2]++;
        }
    }
    lz_quiesce(g.c);
    lzk_guard_release(&g);
    if (rc) return LZ_FRAME_E(GENERIC);
    if (chainErr) result = (size_t)-(long)chainErr;
    else if (j.needHost) { consumed = 0; result = v_finish_on_host(&j, flags, &consumed); }
    else if (j.pendErr) result = j.pendErr;
    else result = j.pos;
    if (LizardGPU_frameIsError(result)) {
        if (!lzk_err()[0]) snprintf(lzk_err(), LZK_ERR_BYTES, "frame refused: %s", LizardF_getErrorName(result));
        return result;
    }
    if (srcConsumedPtr) *srcConsumedPtr = consumed;
    return result;
}

int LizardGPU_frameIndex_device(const void* d_src, size_t srcSize, LizardGPU_frameInfo_t* info, uint64_t* d_payloadOffsets,
                                uint32_t* d_recordWords, size_t maxRecords, size_t* nRecords, size_t* frameBytes, void* stream)
{
    VJob j;
    LzGuard g;
    LzWalkResult r;
    int rc;
    if (nRecords) *nRecords = 0;
    if (frameBytes) *frameBytes = 0;
    lzk_err()[0] = 0;
    if (!d_src && srcSize) return -(int)LIZARDGPU_FRAME_ERR_GENERIC;
    memset(&j, 0, sizeof j);
    memset(&r, 0, sizeof r);
    j.src = (const uint8_t*)d_src; j.srcSize = srcSize; j.B = walk_records();
    lzk_guard_acquire(&g);
    if (g.rc) return -(int)LIZARDGPU_FRAME_ERR_GENERIC;
    j.c = g.c;
    rc = lzk_ctx_init(g.c);
    if (!rc) rc = v_buffers(&j);
    if (!rc) rc = lz_order_after(g.c, (hipStream_t)stream, j.W, j.D, j.C);
    if (!rc) rc = v_issue_walk(&j, 0, 0, (size_t)-1, maxRecords, d_payloadOffsets, d_recordWords);
    if (!rc && hipEventSynchronize(walk_event(&j, 0)) != hipSuccess) { snprintf(lzk_err(), LZK_ERR_BYTES, "the frame walk failed: %s", hipGetErrorString(hipGetLastError())); rc = -LIZARDGPU_ERR_HIP; }
    if (!rc) r = *j.hres[0];
    lz_quiesce(g.c);
    lzk_guard_release(&g);
    if (rc) return -(int)LIZARDGPU_FRAME_ERR_GENERIC;
    if (info && r.infoValid) lz_walk_info(info, &r);
    if (r.status) return -(int)r.status;
    if (nRecords) *nRecords = (size_t)r.nRecords;
    if (frameBytes) *frameBytes = (size_t)r.frameBytes;
    return 0;
}

size_t LizardGPU_frameWalkRecords(void) { return walk_records(); }

size_t LizardGPU_frameBlockSize(unsigned blockSizeID) { return blockSizeID > 7 ? 0 : lzgpu_frame_block_size(blockSizeID); }

int LizardGPU_frameDecodeDeviceStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devFrameStats));
}
