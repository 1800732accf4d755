// unframe_walk.h — device side of LizardGPU_decompressFrame_device / LizardGPU_frameIndex_device (gfx950): the walk over a frame
// that lies in device memory.  One wave does on the device what LizardGPU_frameIndex (lizard_frame_host.c) does on the host, with
// its checks in its order: magic (normal / skippable / unknown), header (version, block-checksum flag, reserved bits, block size
// id, header checksum = XXH32 of at most 11 bytes, restated here in its short-input form only), then the chain of block records
// (one LE32 word per record at an arbitrary byte offset, bounds-checked before it is read; size 0 = end mark; a size above the
// frame's block size or a payload that runs past srcSize = GENERIC), then the 4 checksum bytes the header may ask for.
// The chain is a linked list in memory: every hop is a dependent load, so the walk is one wave, wave-uniform, and works in
// SEGMENTS — from a start position (0 = parse the header first) over at most `budget` records — so that the host can decode segment
// k while segment k + 1 is walked on another stream, and so that the tables stay small for any frame.  Per record the payload's
// offset and the word go to device tables (64 records are collected in the lanes' registers and stored together: a store per hop
// would put its latency into the chain, loads and stores of a wave share one counter); a small result record tells the host how
// the segment ended.
// Every byte of src is read through lz_ld32 / lz_ld8_s, and only inside src[0..srcSize).
// The C part (LzWalkResult) is shared with the host file lizard_unframe_device.c; the body is written against lz_wave.h alone, so
// the CPU SIMT emulator of tests/emul runs it unchanged.
#ifndef LZ_UNFRAME_WALK_H
#define LZ_UNFRAME_WALK_H
#include <stdint.h>

// How a segment ended.  status: 0, or the positive LizardF_ERROR_* number the host walk answers for the same bytes (done = 1 then).
// done = 1 with status 0: the end mark (and the checksum bytes) were in, frameBytes is the frame's size.  done = 0: the budget was
// used up; nextPos is the position of the next record's word.  headerBytes: 7 or 15 (8 for a skippable frame).  The header fields
// are valid when infoValid is set (the host walk fills *info for a skippable frame whose body is cut short, and for a frame whose
// chain is refused).
typedef struct LzWalkResult {
    uint32_t status, done, infoValid, frameType;
    uint32_t blockSizeID, blockMode, checksumFlag, headerBytes;
    uint64_t contentSize, nRecords, nextPos, frameBytes;
} LzWalkResult;

#define LZW_E_GENERIC 1u                 /* LizardF_errorCodes, lib/lizard_frame_static.h:57-67 */
#define LZW_E_MAXBLOCKSIZE 2u
#define LZW_E_VERSION 6u
#define LZW_E_BLOCKCHECKSUM 7u
#define LZW_E_RESERVED 8u
#define LZW_E_HEADER_INCOMPLETE 12u
#define LZW_E_FRAMETYPE 13u
#define LZW_E_HEADERCHECKSUM 17u

#ifdef __cplusplus
#include "lz_wave.h"

// XXH32 (seed 0) of fewer than 16 bytes: no stripe is consumed, so the hash is the tail loop over seed + prime5 + length, then
// the avalanche (xxHash specification; lizard_xxhash.c, Lizard_XXH32_digest with large == 0).
LZ_DEV u32 lz_xxh32_short(const u8* p, u32 len)
{
    u32 h = 374761393u + len, i = 0;
    for (; i + 4u <= len; i += 4u) { h += lz_ld32(p + i) * 3266489917u; h = ((h << 17) | (h >> 15)) * 668265263u; }
    for (; i < len; i++) { h += (u32)lz_ld8_s(p + i) * 374761393u; h = ((h << 11) | (h >> 21)) * 2654435761u; }
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    return h;
}

LZ_DEV u64 lz_walk_block_size(u32 id) { return id < 1u || id > 7u ? 0ull : (id == 1u ? (u64)128 << 10 : (u64)256 << (10u + 2u * (id - 2u))); }

// One segment.  All lanes call; everything is wave-uniform.  startPos 0: the header is parsed and checked first; otherwise it is
// the nextPos of the previous segment of the same frame (whose header has been checked: only its fields are read again).
// offs / words (either may be null) take the first tableCap records of this segment.  Lane 0 writes *res.
LZ_DEV void lz_unframe_walk(const u8* src, u64 srcSize, u64 startPos, u64 budget, u64 tableCap, u64* offs, u32* words, LzWalkResult* res)
{
    const u32 lane = lz_lane();
    u32 status = 0, done = 0, infoValid = 0, frameType = 0, bsid = 0, blockMode = 0, checksumFlag = 0, hSize = 0;
    u64 contentSize = 0, n = 0, pos = startPos, frameBytes = 0;
    do {
        if (srcSize < 5u) { status = LZW_E_HEADER_INCOMPLETE; break; }
        const u32 magic = lz_uniform(lz_ld32(src));
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
            if (srcSize < 8u) { status = LZW_E_HEADER_INCOMPLETE; break; }
            frameType = 1; infoValid = 1; hSize = 8;
            contentSize = lz_uniform(lz_ld32(src + 4));
            if (srcSize - 8u < contentSize) { status = LZW_E_GENERIC; break; }
            frameBytes = 8u + contentSize; done = 1;
            break;
        }
        if (magic != 0x184D2206u) { status = LZW_E_FRAMETYPE; break; }
        const u32 flg = lz_uniform((u32)lz_ld8_s(src + 4));
        hSize = (flg >> 3) & 1u ? 15u : 7u;
        if (srcSize < hSize) { status = LZW_E_HEADER_INCOMPLETE; break; }
        const u32 bd = lz_uniform((u32)lz_ld8_s(src + 5));
        bsid = (bd >> 4) & 7u;
        if (startPos == 0) {                                     // parse_header's checks, in its order
            if (((flg >> 6) & 3u) != 1u) { status = LZW_E_VERSION; break; }
            if ((flg >> 4) & 1u) { status = LZW_E_BLOCKCHECKSUM; break; }
            if (flg & 3u) { status = LZW_E_RESERVED; break; }
            if (bd & 0x80u) { status = LZW_E_RESERVED; break; }
            if (bsid < 1u) { status = LZW_E_MAXBLOCKSIZE; break; }
            if (bd & 0x0Fu) { status = LZW_E_RESERVED; break; }
            const u32 hc = lz_uniform((lz_xxh32_short(src + 4, hSize - 5u) >> 8) & 255u);
            if (hc != lz_uniform((u32)lz_ld8_s(src + hSize - 1u))) { status = LZW_E_HEADERCHECKSUM; break; }
            pos = hSize;
        }
        blockMode = (flg >> 5) & 1u; checksumFlag = (flg >> 2) & 1u; infoValid = 1;
        if (hSize == 15u) contentSize = (u64)lz_uniform(lz_ld32(src + 6)) | ((u64)lz_uniform(lz_ld32(src + 10)) << 32);
        const u64 maxBlock = lz_walk_block_size(bsid);
        u64 offV = 0; u32 wordV = 0;                             // lane l: record (n & ~63) + l of this segment, until it is stored
        while (n < budget) {
            if (srcSize - pos < 4u) { status = LZW_E_GENERIC; break; }
            const u32 word = lz_uniform(lz_ld32(src + pos));
            const u64 size = word & 0x7FFFFFFFu;
            pos += 4u;
            if (size == 0) {                                     // end mark
                if (checksumFlag) {
                    if (srcSize - pos < 4u) { status = LZW_E_GENERIC; break; }
                    pos += 4u;
                }
                frameBytes = pos; done = 1;
                break;
            }
            if (size > maxBlock) { status = LZW_E_GENERIC; break; }
            if (srcSize - pos < size) { status = LZW_E_GENERIC; break; }
            if (lane == (u32)(n & 63u)) { offV = pos; wordV = word; }
            n++;
            pos += size;
            if ((n & 63u) == 0) {
                const u64 at = n - 64u + lane;
                if (at < tableCap) { if (offs) offs[at] = offV; if (words) words[at] = wordV; }
            }
        }
        if (n & 63u) {                                           // the records still in registers (stored on an error too: the host ignores them then)
            const u64 at = (n & ~(u64)63u) + lane;
            if (lane < (u32)(n & 63u) && at < tableCap) { if (offs) offs[at] = offV; if (words) words[at] = wordV; }
        }
    } while (0);
    if (status) done = 1;
    if (lane == 0) {
        res->status = status; res->done = done; res->infoValid = infoValid; res->frameType = frameType;
        res->blockSizeID = bsid; res->blockMode = blockMode; res->checksumFlag = checksumFlag; res->headerBytes = hSize;
        res->contentSize = contentSize; res->nRecords = n; res->nextPos = pos; res->frameBytes = status ? 0 : frameBytes;
    }
}

#ifdef __HIPCC__
struct LzWalkArgs { const u8* src; u64 srcSize, startPos, budget, tableCap; u64* offs; u32* words; LzWalkResult* res; };

__global__ __launch_bounds__(64) void lz_unframe_walk_kernel(LzWalkArgs a)
{
    lz_unframe_walk(a.src, a.srcSize, a.startPos, a.budget, a.tableCap, a.offs, a.words, a.res);
}
#endif
#endif  /* __cplusplus */
#endif
