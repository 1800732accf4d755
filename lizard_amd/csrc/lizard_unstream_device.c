/* lizard_unstream_device.c — LizardGPU_decompressStream_device / LizardGPU_streamIndex_device: a STREAM of frames — back to back in one
 * device buffer, the way the format stores and sends them and the way the reference's CLI appends them, with no table of pointers —
 * decoded into one device buffer in batches (include/lizard_amd.h Part 3b).  Plain C on the HIP runtime's C API and the shim of
 * lizard_gpu_ctx.h, like lizard_unframes_device.c, which does the decoding: this file finds the frames and says where each one goes.
 *
 * The contract is a loop over LizardGPU_decompressFrame_device (pos = out = 0; while pos < srcSize: decode the frame at pos into
 * d_dst + out; stop at an error; out += result, pos += consumed), and the answer is that loop's.  What the loop pays per frame — the
 * context, a walk, a decode and at least three host waits — is paid here per BATCH:
 *   stream walk  lz_unstream_walk_kernel (unstream_kernels.h), one wave, follows the chain of frames from a position and writes one
 *                LzWalkResult and one offset per frame into a table in LzCtx::dfTab; the control record and the table come down in one
 *                copy: one host wait per segment of LIZARDGPU_STREAM_WALK_FRAMES frames.  The table is copied to host memory of the
 *                call's own and kept until it is used up (the batch decoder owns dfTab and the pinned buffers while it runs).
 *   batch        a frame's place in d_dst is the sum of the decoded sizes in front of it, and the header gives a frame's size when it
 *                carries a content size, when the frame is skippable, or when it has no records.  A batch is the longest run of
 *                walked frames in which every frame but the last has such a size (and fits in the room that is left): frame i gets its
 *                size as its capacity, the last gets the real remainder.  The run goes to LizardGPU_decompressFrames_device as it is
 *                (host arrays built from the table; lizard_unframes_device.c is untouched): its two waits.
 *   hand-over    the first frame of the stream that the batch does not answer with exactly its header's size — a frame that is
 *                refused, a chain the walk refuses, a linked frame of more than one record (which the device never settles: it is not
 *                even put into a batch) — is handed to LizardGPU_decompressFrame_device with the loop's own arguments.  An error is
 *                the call's answer; frames behind it are not reported.  Identity with the loop holds by construction there: this file
 *                never re-derives the order of the single entry's refusals.
 * A stream of frames with content sizes (what api.compress_stream_device writes) is ONE batch, however many frames and walk segments
 * it has.  A stream of N frames WITHOUT content sizes degrades to N batches of one frame: correct, and no faster than the loop.  The
 * reference's CLI writes no content size by default; its files are normally one frame, which is one batch.
 *
 * Frames per walk segment: 4 096 by default.  The entry costs 72 bytes (288 KiB of table per segment, on the device and pinned), the
 * segment's host wait is spread over up to 4 096 frame walks, each a chain of dependent loads that costs more than a thousandth of a
 * wait, and a stream shorter than 4 096 * 8 bytes gets a table for (bytes / 8) + 1 frames only — no frame is shorter than 8 bytes. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lizard_amd.h"
#include "lizard_gpu_ctx.h"
#include "lizard_gpu_shim.h"
#include "lizard_device_common.h"
#include "unstream_kernels.h"

#define LZS_WALK_FRAMES   4096
#define LZS_CTL_BYTES     64                                  /* the control record's share of the device / pinned layout */
#define LZS_UNKNOWN       (~(uint64_t)0)

static size_t walk_frames(void)
{
    const char* e = getenv("LIZARDGPU_STREAM_WALK_FRAMES");
    const unsigned long v = e && *e ? strtoul(e, NULL, 10) : 0;
    return v >= 1 && v <= (1ul << 20) ? (size_t)v : LZS_WALK_FRAMES;
}

/* the frames walked so far and not yet used, in host memory of the call's own */
typedef struct {
    const uint8_t* src; size_t srcSize;
    LzWalkResult* w; uint64_t* off;                           /* entries [0, n); at is the next one to use */
    size_t n, at, room;
    size_t end; unsigned why;                                 /* where the last segment stopped and why (LZS_*; 0: nothing walked yet) */
    unsigned long long segments;
} STab;

/* One segment from `pos`, under the context guard: the control record goes up, the walk runs behind what the caller's stream holds, the
 * control record and the table come down: one wait.  The entries are appended to t. */
static int s_segment_locked(LzCtx* c, STab* t, size_t pos, hipStream_t stream)
{
    LzStage* s = c->stage;
    const size_t left = t->srcSize - pos;
    size_t T = walk_frames(), bytes, got;
    LzStreamCtl* h_ctl;
    uint8_t* h_down;
    hipStream_t S;
    int rc;
    if (T > left / 8 + 1) T = left / 8 + 1;
    bytes = LZS_CTL_BYTES + T * (sizeof(LzWalkResult) + 8);
    if ((rc = lzk_ctx_init(c))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&s[0].h_aux, &s[0].h_aux_cap, LZS_CTL_BYTES))) return rc;
    if ((rc = lzp_ensure_pinned((void**)&s[1].h_aux, &s[1].h_aux_cap, bytes))) return rc;
    if ((rc = lzp_ensure_dev(c, (void**)&c->dfTab, &c->dfTabCap, bytes))) return rc;
    if (t->n + T > t->room) {
        const size_t room = t->n + T > 2 * t->room ? t->n + T : 2 * t->room;
        LzWalkResult* w = (LzWalkResult*)realloc(t->w, room * sizeof *w);
        uint64_t* off;
        if (w) t->w = w;
        off = w ? (uint64_t*)realloc(t->off, room * sizeof *off) : NULL;
        if (off) t->off = off;
        if (!w || !off) { snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); return -LIZARDGPU_ERR_NOMEM; }
        t->room = room;
    }
    h_ctl = (LzStreamCtl*)s[0].h_aux; h_down = s[1].h_aux; S = s[1].stream;
    memset(h_ctl, 0, LZS_CTL_BYTES);
    h_ctl->pos = (uint64_t)pos;
    c->hostKernelMs = -1.0f;
    LZ_HIP(hipEventRecord(s[0].up, stream));
    LZ_HIP(hipStreamWaitEvent(S, s[0].up, 0));
    LZ_HIP(hipMemcpyAsync(c->dfTab, h_ctl, LZS_CTL_BYTES, hipMemcpyHostToDevice, S));
    if ((rc = lzk_unstream_walk_launch(t->src, t->srcSize, (LzStreamCtl*)c->dfTab, (LzWalkResult*)(c->dfTab + LZS_CTL_BYTES),
                                       (uint64_t*)(c->dfTab + LZS_CTL_BYTES + T * sizeof(LzWalkResult)), (uint32_t)T, S))) return rc;
    LZ_HIP(hipMemcpyAsync(h_down, c->dfTab, bytes, hipMemcpyDeviceToHost, S));
    LZ_HIP(hipEventRecord(s[0].meta, S));
    LZ_HIP(hipEventSynchronize(s[0].meta));
    h_ctl = (LzStreamCtl*)h_down;
    got = (size_t)h_ctl->nFrames;
    if (got > T || h_ctl->why < LZS_END || h_ctl->why > LZS_REFUSED || h_ctl->pos > (uint64_t)t->srcSize || (!got && h_ctl->why != LZS_END)) {
        snprintf(lzk_err(), LZK_ERR_BYTES, "the stream walk left an impossible control record");
        return -LIZARDGPU_ERR_HIP;
    }
    memcpy(t->w + t->n, h_down + LZS_CTL_BYTES, got * sizeof(LzWalkResult));
    memcpy(t->off + t->n, h_down + LZS_CTL_BYTES + T * sizeof(LzWalkResult), got * 8);
    t->n += got; t->end = (size_t)h_ctl->pos; t->why = h_ctl->why;
    t->segments++;
    return 0;
}

static int s_segment(STab* t, size_t pos, hipStream_t stream)
{
    LzGuard g;
    int rc;
    lzk_guard_acquire(&g);
    if (g.rc) return g.rc;
    rc = s_segment_locked(g.c, t, pos, stream);
    if (rc) lz_quiesce(g.c);                                   /* (a segment that succeeded ended in its one wait: nothing is in flight) */
    lzk_guard_release(&g);
    return rc;
}

static void s_forget(STab* t) { t->n = t->at = 0; t->why = 0; }
/* entry i is the one a segment stopped at with LZS_REFUSED: not an accepted frame, whatever its status says (the kernel also stops at
 * a length that is 0 or runs past the stream, which lz_unframe_walk never reports today) */
static int s_refused(const STab* t, size_t i) { return t->w[i].status || (t->why == LZS_REFUSED && i + 1 == t->n); }
static void s_free(STab* t) { free(t->w); free(t->off); t->w = NULL; t->off = NULL; }

/* the decoded size the header promises, or LZS_UNKNOWN */
static uint64_t s_known(const LzWalkResult* w)
{
    if (w->frameType || !w->nRecords) return 0;
    return w->contentSize ? w->contentSize : LZS_UNKNOWN;
}

static void s_stats_add(const unsigned long long add[4])       /* the error text survives */
{
    char keep[LZK_ERR_BYTES];
    LzCtx* c;
    int i;
    lz_err_save(keep);
    if ((c = lzk_ctx_peek())) {
        pthread_mutex_lock(&c->mu);
        for (i = 0; i < 4; i++) c->devStreamDecodeStats[i] += add[i];
        pthread_mutex_unlock(&c->mu);
    }
    lz_err_restore(keep);
}

static void s_name_failure(int rc)                             /* a failure of the machinery never leaves without a text */
{
    if (!lzk_err()[0]) snprintf(lzk_err(), LZK_ERR_BYTES, "the stream decoder's machinery failed (LIZARDGPU_ERR %d)", -rc);
}

/* the host arrays of one batch */
typedef struct { void** dsts; const void** srcs; size_t *caps, *sizes, *results, *used; size_t room; } SBatch;
static int s_batch_room(SBatch* b, size_t n)
{
    if (n <= b->room) return 0;
    free(b->dsts); free((void*)b->srcs); free(b->caps);
    b->room = 0;
    b->dsts = (void**)malloc(n * sizeof(void*)); b->srcs = (const void**)malloc(n * sizeof(void*));
    b->caps = (size_t*)malloc(4 * n * sizeof(size_t));
    if (!b->dsts || !b->srcs || !b->caps) { snprintf(lzk_err(), LZK_ERR_BYTES, "out of host memory"); return -LIZARDGPU_ERR_NOMEM; }
    b->sizes = b->caps + n; b->results = b->sizes + n; b->used = b->results + n;
    b->room = n;
    return 0;
}
static void s_batch_free(SBatch* b) { free(b->dsts); free((void*)b->srcs); free(b->caps); memset(b, 0, sizeof *b); }

size_t LizardGPU_decompressStream_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr,
                                         size_t* nFramesPtr, size_t* decodedPtr, unsigned flags, void* stream)
{
    STab t;
    SBatch b;
    unsigned long long stats[4] = { 0, 0, 0, 0 };
    size_t pos = 0, out = 0, frames = 0, answer = 0;
    int rc = 0, stop = 0;
    if (!srcSize) return 0;
    lzk_err()[0] = 0;
    if (srcConsumedPtr) *srcConsumedPtr = 0;
    if (nFramesPtr) *nFramesPtr = 0;
    if (decodedPtr) *decodedPtr = 0;
    if ((!d_dst && dstCapacity) || !d_src) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null pointer)"); return LZ_FRAME_E(GENERIC); }
    memset(&t, 0, sizeof t);
    memset(&b, 0, sizeof b);
    t.src = (const uint8_t*)d_src; t.srcSize = srcSize;
    while (pos < srcSize && !stop) {
        size_t n = 0, place = 0, i;
        int single;
        if (t.at == t.n) {                                     /* nothing walked ahead: the next segment starts at pos */
            s_forget(&t);
            if ((rc = s_segment(&t, pos, (hipStream_t)stream))) break;
        }
        /* the run: from t.at, every frame but the last with a size the header gives and room for it; more segments while it goes on */
        for (;;) {
            const LzWalkResult* w;
            uint64_t known;
            if (t.at + n == t.n) {
                if (t.why != LZS_FULL) break;
                if ((rc = s_segment(&t, t.end, (hipStream_t)stream))) break;
                continue;
            }
            w = &t.w[t.at + n];
            if (s_refused(&t, t.at + n) || (!w->frameType && !w->blockMode && w->nRecords > 1)) break;      /* the single entry's, in front of it the run ends */
            n++;
            known = s_known(w);
            if (known == LZS_UNKNOWN || known > (uint64_t)(dstCapacity - out - place)) break;  /* the run's last: it gets the real remainder */
            place += (size_t)known;
        }
        if (rc) break;
        single = n == 0;
        if (n) {
            if ((rc = s_batch_room(&b, n))) break;
            place = 0;
            for (i = 0; i < n; i++) {
                const LzWalkResult* w = &t.w[t.at + i];
                const uint64_t known = s_known(w);
                b.srcs[i] = t.src + t.off[t.at + i]; b.sizes[i] = (size_t)w->frameBytes;
                b.dsts[i] = d_dst ? (uint8_t*)d_dst + out + place : NULL;
                b.caps[i] = i + 1 < n ? (size_t)known : dstCapacity - out - place;
                place += i + 1 < n ? (size_t)known : 0;
            }
            rc = LizardGPU_decompressFrames_device(n, b.dsts, b.caps, b.srcs, b.sizes, b.results, b.used, flags, stream);
            if (rc) break;
            stats[1]++;
            for (i = 0; i < n; i++) {
                const LzWalkResult* w = &t.w[t.at];
                const uint64_t known = s_known(w);
                if (LizardGPU_frameIsError(b.results[i]) || b.used[i] != (size_t)w->frameBytes || (known != LZS_UNKNOWN && b.results[i] != (size_t)known)) { single = 1; break; }
                out += b.results[i]; pos += b.used[i]; frames++; t.at++;
                stats[0]++;
            }
        }
        if (single && pos < srcSize) {                         /* the loop's own call for the frame at pos */
            size_t used = 0;
            const size_t r = LizardGPU_decompressFrame_device(d_dst ? (uint8_t*)d_dst + out : NULL, dstCapacity - out, t.src + pos, srcSize - pos, &used,
                                                              flags, stream);
            stats[2]++;
            if (LizardGPU_frameIsError(r)) { answer = r; stop = 1; break; }
            if (t.at < t.n && !s_refused(&t, t.at) && used == (size_t)t.w[t.at].frameBytes) t.at++;      /* the table still holds */
            else s_forget(&t);
            out += r; pos += used; frames++;
            if (!used) { snprintf(lzk_err(), LZK_ERR_BYTES, "the single-frame entry consumed nothing"); rc = -LIZARDGPU_ERR_HIP; break; }
        }
    }
    stats[3] = t.segments;
    s_free(&t);
    s_batch_free(&b);
    s_stats_add(stats);
    if (srcConsumedPtr) *srcConsumedPtr = pos;
    if (nFramesPtr) *nFramesPtr = frames;
    if (decodedPtr) *decodedPtr = out;
    if (rc) { s_name_failure(rc); return LZ_FRAME_E(GENERIC); }
    if (stop) return answer;
    lzk_err()[0] = 0;
    return out;
}

int LizardGPU_streamIndex_device(const void* d_src, size_t srcSize, uint64_t* frameOffsets, uint64_t* frameBytes, LizardGPU_frameInfo_t* infos,
                                 size_t* nRecords, size_t maxFrames, size_t* nFrames, size_t* streamBytes, void* stream)
{
    STab t;
    unsigned long long stats[4] = { 0, 0, 0, 0 };
    size_t pos = 0, count = 0, i;
    int rc = 0, code = 0;
    if (nFrames) *nFrames = 0;
    if (streamBytes) *streamBytes = 0;
    lzk_err()[0] = 0;
    if (!srcSize) return 0;
    if (!d_src) { snprintf(lzk_err(), LZK_ERR_BYTES, "bad argument (null pointer)"); return -(int)LIZARDGPU_FRAME_ERR_GENERIC; }
    memset(&t, 0, sizeof t);
    t.src = (const uint8_t*)d_src; t.srcSize = srcSize;
    while (pos < srcSize && !code) {
        s_forget(&t);
        if ((rc = s_segment(&t, pos, (hipStream_t)stream))) break;
        for (i = 0; i < t.n; i++) {
            const LzWalkResult* w = &t.w[i];
            if (count < maxFrames && infos && w->infoValid) lz_walk_info(&infos[count], w);
            if (s_refused(&t, i)) { code = -(int)(w->status ? w->status : LIZARDGPU_FRAME_ERR_GENERIC); break; }
            if (count < maxFrames) {
                if (frameOffsets) frameOffsets[count] = t.off[i];
                if (frameBytes) frameBytes[count] = w->frameBytes;
                if (nRecords) nRecords[count] = (size_t)w->nRecords;
            }
            count++;
        }
        pos = t.end;
    }
    stats[3] = t.segments;
    s_free(&t);
    s_stats_add(stats);
    if (rc) { s_name_failure(rc); return -(int)LIZARDGPU_FRAME_ERR_GENERIC; }
    if (nFrames) *nFrames = count;
    if (streamBytes) *streamBytes = pos;
    if (code) snprintf(lzk_err(), LZK_ERR_BYTES, "frame %zu at offset %zu refused: %s", count, pos, LizardF_getErrorName((size_t)(long)code));
    return code;
}

int LizardGPU_streamDecodeDeviceStats(unsigned long long out[4])
{
    return lz_stats_read(out, offsetof(LzCtx, devStreamDecodeStats));
}
