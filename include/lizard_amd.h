/*
 * lizard_amd.h — C ABI of liblizard_amd.so, the MI355X-native Lizard block-compress path.
 *
 * The library is a link-time replacement of the reference's liblizard: it exports every symbol of
 * lib/dll/liblizard.def, of lib/lizard_frame.h and the Lizard_XXH* hash functions the reference's programs use, with the
 * reference's names, argument meaning and error behaviour — the sources under programs/, tests/fuzzer.c, tests/frametest.c and
 * tests/fullbench.c link against it with no reference object at all (oracle/Makefile) — plus the LizardGPU_*
 * extension.  Each entry cites the reference declaration it replaces.
 *   Part 1   block compression      lib/lizard_compress.h       on the GPU, no host path
 *   Part 1b  block decompression    lib/lizard_decompress.h     one block per call: on the calling thread (not the accelerated path)
 *   Part 1c  frames                 lib/lizard_frame.h          compression batched on the GPU; LizardF_decompress on the host
 *                                                               (a whole frame in one call on the GPU: LizardGPU_decompressFrame, Part 3b)
 *   Part 1d  XXH32 / XXH64          lib/xxhash/xxhash.h         (XXH_NAMESPACE=Lizard_, lib/Makefile:52)
 *   Part 2   batch extension (ours): many independent blocks per call, host- or device-resident, several GPUs, decompression
 *   Part 3   the strict frame twins of rounds 2-3 (LizardGPU_compressFrame ...) and their forms for data in device memory: one frame
 *            (LizardGPU_compressFrame_device), a batch (LizardGPU_compressFrames_device), a batch written back to back into one
 *            buffer, a .liz stream (LizardGPU_compressStream_device, LizardGPU_compressStreamBound)
 *   Part 3b  whole-frame decompression on the GPU (LizardGPU_decompressFrame, LizardGPU_decompressFrame_device,
 *            LizardGPU_decompressFrames_device, LizardGPU_decompressStream_device ...)
 *   Part 3c  tensor streams: element bytes split into planes before compressing (LizardGPU_splitPlanes_device,
 *            LizardGPU_joinPlanes_device) or, opt-in, element bits (LizardGPU_splitBitPlanes_device, LizardGPU_joinBitPlanes_device),
 *            either of them after an XOR with an earlier version of the buffer, opt-in and per buffer
 *            (LizardGPU_splitPlanesXor_device, LizardGPU_joinPlanesXor_device), and the tensor header, a skippable frame
 *            (LizardGPU_tensorHeaderWrite / Read, with a filter: Write2 / Read2, with a base: Write3 / Read3)
 *   Part 3d  a row range of a tensor decoded from the blocks that cover it (LizardGPU_planesRangeBytes,
 *            LizardGPU_decompressFrameRanges_device, LizardGPU_joinPlanesRange_device)
 *
 * Plain C, plain pointers and sizes; no HIP or torch types in any signature (a HIP stream is passed
 * as an opaque void*).
 */
#ifndef LIZARD_AMD_H
#define LIZARD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================= Part 1: reference block API (lib/lizard_compress.h) ======================= */

#define LIZARD_MIN_CLEVEL      10            /* reference lib/lizard_compress.h:86 */
#define LIZARD_MAX_CLEVEL      49            /* reference lib/lizard_compress.h:88 */
#define LIZARD_DEFAULT_CLEVEL  17            /* reference lib/lizard_compress.h:92 */
#define LIZARD_MAX_INPUT_SIZE  0x7E000000    /* reference lib/lizard_compress.h:121 */
#define LIZARD_BLOCK_SIZE      (1<<17)       /* reference lib/lizard_compress.h:122 */
#define LIZARD_COMPRESSBOUND(isize)  ((unsigned)(isize) > (unsigned)LIZARD_MAX_INPUT_SIZE ? 0 : (isize) + 1 + 1 + ((isize/LIZARD_BLOCK_SIZE)+1)*4)   /* :124 */

typedef struct Lizard_stream_s Lizard_stream_t;   /* opaque, reference lib/lizard_compress.h:94 */

/* reference lib/lizard_compress.h:66 / lib/lizard_compress.c:66 */
int Lizard_versionNumber(void);

/* reference lib/lizard_compress.h:99 / lib/lizard_compress.c:596.
 * Returns bytes written into dst, 0 on failure (dst too small, level not accelerated, GPU error).
 * Never writes past dst+maxDstSize, never reads outside src[0..srcSize).  (maxDstSize <= 0 returns 0, where the
 * reference's room test wraps, lizard_compress.c:238/:489, and it writes past the buffer — with the one exception its own
 * frame layer produces: a 1-byte block with maxDstSize 0 (lizard_frame.c:461) returns the reference's 6 bytes.) */
int Lizard_compress(const char* src, char* dst, int srcSize, int maxDstSize, int compressionLevel);

/* reference lib/lizard_compress.h:135 / lib/lizard_compress.c:67 */
int Lizard_compressBound(int inputSize);

/* reference lib/lizard_compress.h:145-147 / lib/lizard_compress.c:311,583.
 * `state` must be pointer-aligned (misaligned => 0, as the reference) and Lizard_sizeofState(level)
 * bytes; its content on entry is irrelevant (the reference re-initialises it on every call, and the
 * match-finder tables of this implementation live on the device). */
int Lizard_sizeofState(int compressionLevel);
int Lizard_compress_extState(void* state, const char* src, char* dst, int srcSize, int maxDstSize, int compressionLevel);

/* reference lib/lizard_compress.h:159-160,166 / lib/lizard_compress.c:392,417,401 */
Lizard_stream_t* Lizard_createStream(int compressionLevel);
int              Lizard_freeStream(Lizard_stream_t* streamPtr);
Lizard_stream_t* Lizard_resetStream(Lizard_stream_t* streamPtr, int compressionLevel);

/* reference lib/lizard_common.h:493-497 / lib/lizard_compress.c:68,612-630 (level-10 aliases) */
int Lizard_sizeofState_MinLevel(void);
int Lizard_compress_MinLevel(const char* source, char* dest, int sourceSize, int maxDestSize);
int Lizard_compress_extState_MinLevel(void* state, const char* source, char* dest, int inputSize, int maxDestSize);
Lizard_stream_t* Lizard_resetStream_MinLevel(Lizard_stream_t* streamPtr);
Lizard_stream_t* Lizard_createStream_MinLevel(void);

/* reference lib/lizard_compress.h:178,198,188 / lib/lizard_compress.c:426,454,550 — streaming ("linked blocks") and
 * dictionaries.  In the reference a stream is one serial chain (hash table, window and repeat offset carried from call to
 * call) — nothing a GPU can parallelise.  Implemented HISTORY-FREE: Lizard_compress_continue compresses its block on the GPU
 * without referring to earlier data (same return contract as Lizard_compress_extState at the stream's level); loadDict and
 * saveDict do the reference's book-keeping (returned sizes; saveDict copies the last min(dictSize, prefix) bytes of the
 * previous block into safeBuffer).  Every block is valid for Lizard_decompress_safe_continue / _usingDict — a decoder never
 * requires a block to use its history — so frames in the frame layer's default linked mode are compressed and decodable;
 * their bytes are those of independent blocks, not the reference's linked-mode bytes. */
int Lizard_loadDict(Lizard_stream_t* streamPtr, const char* dictionary, int dictSize);
int Lizard_saveDict(Lizard_stream_t* streamPtr, char* safeBuffer, int dictSize);
int Lizard_compress_continue(Lizard_stream_t* streamPtr, const char* src, char* dst, int srcSize, int maxDstSize);

/* ======================= Part 1b: reference block decompression (lib/lizard_decompress.h) =======================
 * One block per call, on the calling thread (lizard_amd/csrc/lizard_decode_host.c): the decoder is not the path this library
 * accelerates, and one block is ~0.1 ms of host work against ~1 ms as a single wavefront.  Many independent blocks:
 * LizardGPU_decompressBlocks_host / _device below.  Same results as the reference for every VALID block (every block a Lizard
 * compressor produces: offsets >= 8).  Malformed input is refused (negative result) without reading outside
 * source[0..compressedSize) or writing outside dest[0..maxDecompressedSize) — and that is where the identity ends: an offset of
 * 0 is refused here, offsets 1..7 copy with true LZ overlap semantics (the reference's 8- and 16-byte wild copies produce a
 * different byte pattern for them), and a literal run that overruns the literals stream is refused (the reference has no such
 * test).  tests/decode_fuzz.c runs the decoder under ASan / UBSan on damaged blocks. */
typedef struct Lizard_streamDecode_s Lizard_streamDecode_t;   /* 4 words, valid when zeroed (reference lib/lizard_common.h:195-200) */
/* reference lib/lizard_decompress.h:64 / lib/lizard_decompress.c:267 */
int Lizard_decompress_safe(const char* source, char* dest, int compressedSize, int maxDecompressedSize);
/* reference lib/lizard_decompress.h:80 / lib/lizard_decompress.c:272: may stop once targetOutputSize bytes exist (returns >= that) */
int Lizard_decompress_safe_partial(const char* source, char* dest, int compressedSize, int targetOutputSize, int maxDecompressedSize);
/* reference lib/lizard_decompress.h:102-103,110 / lib/lizard_decompress.c:288-314 */
Lizard_streamDecode_t* Lizard_createStreamDecode(void);
int Lizard_freeStreamDecode(Lizard_streamDecode_t* Lizard_stream);
int Lizard_setStreamDecode(Lizard_streamDecode_t* Lizard_streamDecode, const char* dictionary, int dictSize);
/* reference lib/lizard_decompress.h:131 / lib/lizard_decompress.c:325: previous output is the history (prefix if contiguous) */
int Lizard_decompress_safe_continue(Lizard_streamDecode_t* Lizard_streamDecode, const char* source, char* dest, int compressedSize, int maxDecompressedSize);
/* reference lib/lizard_decompress.h:142 / lib/lizard_decompress.c:360, :374 */
int Lizard_decompress_safe_usingDict(const char* source, char* dest, int compressedSize, int maxDecompressedSize, const char* dictStart, int dictSize);
int Lizard_decompress_safe_forceExtDict(const char* source, char* dest, int compressedSize, int maxOutputSize, const char* dictStart, int dictSize);

/* ======================= Part 1c: reference frame API (lib/lizard_frame.h) =======================
 * Types as lib/lizard_frame.h:59-234 declares them (define LIZARD_AMD_NO_FRAME_TYPES before this header when the reference's
 * lizard_frame.h is included too).  Compression: every run of blocks an Update / compressFrame call covers is ONE batch on the
 * GPU (lizard_amd/csrc/lizard_frame_host.c).  Independent blocks: byte for byte the reference's frames (zero-state build).
 * Linked blocks: valid frames whose blocks do not use their history (Lizard_compress_continue above).  A level without a GPU
 * kernel or a GPU failure stores the blocks raw, as the reference's frame layer does when Lizard_compress_extState returns 0
 * (lib/lizard_frame.c:456-469), after a line on stderr. */
#ifndef LIZARD_AMD_NO_FRAME_TYPES
typedef size_t LizardF_errorCode_t;
typedef enum { LizardF_default = 0, LizardF_max128KB = 1, LizardF_max256KB = 2, LizardF_max1MB = 3, LizardF_max4MB = 4,
               LizardF_max16MB = 5, LizardF_max64MB = 6, LizardF_max256MB = 7 } LizardF_blockSizeID_t;
typedef enum { LizardF_blockLinked = 0, LizardF_blockIndependent } LizardF_blockMode_t;
typedef enum { LizardF_noContentChecksum = 0, LizardF_contentChecksumEnabled } LizardF_contentChecksum_t;
typedef enum { LizardF_frame = 0, LizardF_skippableFrame } LizardF_frameType_t;
typedef struct {
    LizardF_blockSizeID_t     blockSizeID;          /* 0 = default (128 KiB) */
    LizardF_blockMode_t       blockMode;            /* 0 = linked (default), 1 = independent */
    LizardF_contentChecksum_t contentChecksumFlag;
    LizardF_frameType_t       frameType;
    unsigned long long        contentSize;          /* != 0: the header carries the content size */
    unsigned                  reserved[2];
} LizardF_frameInfo_t;                              /* lib/lizard_frame.h:111-118 */
typedef struct {
    LizardF_frameInfo_t frameInfo;
    int      compressionLevel;                      /* clamped like Lizard_createStream (lib/lizard_compress.c:303-308) */
    unsigned autoFlush;                             /* 1 = every Update call ends on a block boundary (no buffering) */
    unsigned reserved[4];
} LizardF_preferences_t;                            /* lib/lizard_frame.h:120-125 */
typedef struct LizardF_cctx_s* LizardF_compressionContext_t;      /* lib/lizard_frame.h:148 */
typedef struct { unsigned stableSrc; unsigned reserved[3]; } LizardF_compressOptions_t;      /* :150-154 */
typedef struct LizardF_dctx_s* LizardF_decompressionContext_t;    /* :229 */
typedef struct { unsigned stableDst; unsigned reserved[3]; } LizardF_decompressOptions_t;    /* :231-234 */
#define LIZARDF_VERSION 100
#endif
/* reference lib/lizard_frame.h:59-60 / lib/lizard_frame.c:179-189; codes are (size_t)-LizardF_ERROR_* (lib/lizard_frame_static.h:57-67) */
unsigned    LizardF_isError(size_t code);
const char* LizardF_getErrorName(size_t code);
/* reference lib/lizard_frame.h:131,143 / lib/lizard_frame.c:229,260 */
size_t LizardF_compressFrameBound(size_t srcSize, const LizardF_preferences_t* preferencesPtr);
size_t LizardF_compressFrame(void* dstBuffer, size_t dstMaxSize, const void* srcBuffer, size_t srcSize, const LizardF_preferences_t* preferencesPtr);
/* reference lib/lizard_frame.h:159-160,172,181,193,205,216 / lib/lizard_frame.c:329,346,362,432,501,610,651 */
size_t LizardF_createCompressionContext(LizardF_compressionContext_t* cctxPtr, unsigned version);
size_t LizardF_freeCompressionContext(LizardF_compressionContext_t cctx);
size_t LizardF_compressBegin(LizardF_compressionContext_t cctx, void* dstBuffer, size_t dstMaxSize, const LizardF_preferences_t* prefsPtr);
size_t LizardF_compressBound(size_t srcSize, const LizardF_preferences_t* prefsPtr);
size_t LizardF_compressUpdate(LizardF_compressionContext_t cctx, void* dstBuffer, size_t dstMaxSize, const void* srcBuffer, size_t srcSize,
                              const LizardF_compressOptions_t* cOptPtr);
size_t LizardF_flush(LizardF_compressionContext_t cctx, void* dstBuffer, size_t dstMaxSize, const LizardF_compressOptions_t* cOptPtr);
size_t LizardF_compressEnd(LizardF_compressionContext_t cctx, void* dstBuffer, size_t dstMaxSize, const LizardF_compressOptions_t* cOptPtr);
/* reference lib/lizard_frame.h:247-248,265,297 / lib/lizard_frame.c:689,699,871,980.  Blocks are decoded by Part 1b's decoder;
 * the context keeps the 16 MiB history of a linked frame itself (stableDst is accepted and not needed). */
size_t LizardF_createDecompressionContext(LizardF_decompressionContext_t* dctxPtr, unsigned version);
size_t LizardF_freeDecompressionContext(LizardF_decompressionContext_t dctx);
size_t LizardF_getFrameInfo(LizardF_decompressionContext_t dctx, LizardF_frameInfo_t* frameInfoPtr, const void* srcBuffer, size_t* srcSizePtr);
size_t LizardF_decompress(LizardF_decompressionContext_t dctx, void* dstBuffer, size_t* dstSizePtr, const void* srcBuffer, size_t* srcSizePtr,
                          const LizardF_decompressOptions_t* dOptPtr);

/* ======================= Part 1d: XXH32 / XXH64 (lib/xxhash/xxhash.h with XXH_NAMESPACE=Lizard_) =======================
 * programs/bench.c, tests/fuzzer.c and tests/frametest.c call these; the state structs are the caller's (the reference's
 * XXH32_state_t / XXH64_state_t: 48 / 88 bytes), this library's layouts fit inside them.  XXH_errorcode: 0 = ok. */
struct Lizard_XXH32_state_s; struct Lizard_XXH64_state_s;
unsigned Lizard_XXH_versionNumber(void);
unsigned Lizard_XXH32(const void* input, size_t length, unsigned seed);                                   /* xxhash.h:167 */
struct Lizard_XXH32_state_s* Lizard_XXH32_createState(void);                                             /* :171-177 */
int      Lizard_XXH32_freeState(struct Lizard_XXH32_state_s* statePtr);
void     Lizard_XXH32_copyState(struct Lizard_XXH32_state_s* dst, const struct Lizard_XXH32_state_s* src);
int      Lizard_XXH32_reset(struct Lizard_XXH32_state_s* statePtr, unsigned seed);
int      Lizard_XXH32_update(struct Lizard_XXH32_state_s* statePtr, const void* input, size_t length);
unsigned Lizard_XXH32_digest(const struct Lizard_XXH32_state_s* statePtr);
void     Lizard_XXH32_canonicalFromHash(unsigned char* dst, unsigned hash);                              /* :204-205 (big-endian bytes) */
unsigned Lizard_XXH32_hashFromCanonical(const unsigned char* src);
unsigned long long Lizard_XXH64(const void* input, size_t length, unsigned long long seed);              /* :225 */
struct Lizard_XXH64_state_s* Lizard_XXH64_createState(void);                                             /* :229-235 */
int      Lizard_XXH64_freeState(struct Lizard_XXH64_state_s* statePtr);
void     Lizard_XXH64_copyState(struct Lizard_XXH64_state_s* dst, const struct Lizard_XXH64_state_s* src);
int      Lizard_XXH64_reset(struct Lizard_XXH64_state_s* statePtr, unsigned long long seed);
int      Lizard_XXH64_update(struct Lizard_XXH64_state_s* statePtr, const void* input, size_t length);
unsigned long long Lizard_XXH64_digest(const struct Lizard_XXH64_state_s* statePtr);
void     Lizard_XXH64_canonicalFromHash(unsigned char* dst, unsigned long long hash);                    /* :239-240 */
unsigned long long Lizard_XXH64_hashFromCanonical(const unsigned char* src);

/* ======================= Part 2: batch extension (ours) ======================= */

/* Error codes returned (negated) by the LizardGPU_* entry points. */
enum {
    LIZARDGPU_OK = 0,
    LIZARDGPU_ERR_NO_DEVICE = 1,     /* no HIP device / HIP runtime failure at init */
    LIZARDGPU_ERR_LEVEL = 2,         /* level not implemented on the GPU path */
    LIZARDGPU_ERR_ARG = 3,           /* bad size / stride / null pointer */
    LIZARDGPU_ERR_HIP = 4,           /* a HIP call failed (see LizardGPU_lastError) */
    LIZARDGPU_ERR_NOMEM = 5,         /* device or pinned-host allocation failed */
    LIZARDGPU_ERR_RCCL = 6,          /* RCCL could not be loaded or a collective failed */
    LIZARDGPU_ERR_HARDWARE = 7       /* the device failed the library's self-check of a property the level's kernel relies on:
                                      * lanes of one LDS atomic that hit the same dword are served in ascending lane order
                                      * (checked once per device at context creation; levels 10/30 and the hashChain levels) */
};

/* 1 if `compressionLevel` (after the reference's clamp, lib/lizard_compress.c:303-308) runs on the GPU:
 * 10 (fastSmall), 11 (fast), 12 (noChain), 13..17 (hashChain), 20 (fastBig), 21, 22 (priceFast) and their huff0 twins 30, 31, 32, 33,
 * 34..38, 40, 41, 42 — every row of Lizard_defaultParameters (lib/lizard_common.h:234-284) whose parser is fastSmall, fast, noChain, hashChain,
 * fastBig or priceFast (23 of the 40 levels; the others are the price-based parsers),
 * at every block size the reference takes (LIZARD_MAX_INPUT_SIZE, lib/lizard_compress.h:121). */
int LizardGPU_levelSupported(int compressionLevel);
/* Largest block (bytes) the GPU path takes at this level: LIZARD_MAX_INPUT_SIZE, or 0 if the level has no GPU kernel. */
size_t LizardGPU_maxBlockSize(int compressionLevel);

/* Devices.  The library keeps one context per device (arenas, tables, streams, pinned staging), created on first
 * use and serialised by its own lock; host threads working on different devices run concurrently.
 * LizardGPU_setDevice selects the device for the CALLING THREAD's later calls and becomes the default of threads
 * that never selected one (initially device 0); an index outside 0..deviceCount-1 is refused (-LIZARDGPU_ERR_ARG).
 * Every entry point makes its device current for the duration of the call and restores the caller's.
 * LizardGPU_shutdown releases every device allocation, stream, pinned buffer and RCCL communicator of the
 * process (synchronises the devices first); the next call re-creates what it needs. */
int  LizardGPU_deviceCount(void);
int  LizardGPU_setDevice(int device);
void LizardGPU_shutdown(void);

/* Text of the calling thread's last failure ("" after a successful call; thread-local storage). */
const char* LizardGPU_lastError(void);

/* Compress nBlocks independent blocks that are already RESIDENT IN DEVICE MEMORY.
 *   d_src      : device pointer, block i starts at d_src + i*blockSize; every block is blockSize bytes
 *                except the last, which is lastBlockSize (1..blockSize)
 *   d_dst      : device pointer, block i's output starts at d_dst + i*dstStride;
 *                dstStride >= Lizard_compressBound(blockSize)
 *   d_sizes    : device pointer to nBlocks uint32: compressed size of each block (never 0: with a
 *                bound-sized slot compression cannot fail, reference lib/lizard_compress.h:104)
 *   level      : 10..49, must satisfy LizardGPU_levelSupported
 *   stream     : hipStream_t as void* (NULL = default stream). The call only enqueues work; outputs are
 *                valid after the stream is synchronised.  Launches of one process share the per-wave scratch
 *                arena and the tables: a launch on a different stream waits on the device for the previous
 *                one (stream-ordered, no host synchronisation).
 * Each block is what Lizard_compress_extState() produces on a zero-initialised state
 * (reference lib/lizard_compress.c:583 built with -DLIZARD_RESET_MEM). Returns 0 or -LIZARDGPU_ERR_*. */
int LizardGPU_compressBlocks_device(const void* d_src, size_t nBlocks, size_t blockSize, size_t lastBlockSize,
                                    void* d_dst, size_t dstStride, uint32_t* d_sizes,
                                    int level, void* stream);

/* Same for HOST-resident buffers (dst slot i at dst + i*dstStride, cSizes[i] bytes valid).  Synchronous.
 * Pipelined in chunks of whole blocks (256 MiB of input, LIZARDGPU_CHUNK_MB overrides), three chunks in flight: pinned
 * staging, H2D, kernels, device-side compaction of the valid bytes, ONE D2H per chunk.  The calling thread stages and issues,
 * a second host thread (alive for the duration of the call) drains: uploads, kernels, downloads and the host copies of
 * different chunks run side by side.  A src that is already pinned (hipHostMalloc / hipHostRegister) is read by DMA directly.
 * _host_packed writes the compressed blocks back to back instead: block i at dst + offsets[i], cSizes[i] bytes,
 * offsets[nBlocks] = total (offsets / cSizes may be NULL); -LIZARDGPU_ERR_ARG if dstCapacity is too small. */
int LizardGPU_compressBlocks_host(const void* src, size_t nBlocks, size_t blockSize, size_t lastBlockSize,
                                  void* dst, size_t dstStride, uint32_t* cSizes, int level);
int LizardGPU_compressBlocks_host_packed(const void* src, size_t nBlocks, size_t blockSize, size_t lastBlockSize,
                                         void* dst, size_t dstCapacity, uint64_t* offsets, uint32_t* cSizes, int level);

/* ---- several GPUs ----
 * Blocks are independent: rank r of R owns the contiguous range LizardGPU_shardRange gives it, no halo; the one
 * exchange is the RCCL all-gather of the per-block compressed sizes (uint32 per block, over xGMI inside a node),
 * followed by an exclusive prefix sum = byte offset of every block in the concatenated output.
 *
 * One process driving nDevices GPUs: device devices[r] (r if devices == NULL) holds its blocks back to back at d_src[r]
 * and gets its slots at d_dst[r]; on return (synchronous) every device's d_allSizes[r][0..nBlocks) holds ALL sizes
 * and d_offsets[r][0..nBlocks] the offsets (last entry = total).  The ragged last block belongs to the last rank.
 *
 * One process per GPU (torchrun): rank 0 calls LizardGPU_commUniqueId (128 bytes), the launcher's transport carries
 * them to the other ranks, every rank calls LizardGPU_commInitRank once, then LizardGPU_gatherSizes_device after each
 * batch: d_localSizes = this rank's shard (may already sit at d_allSizes + first), enqueued on `stream`.
 * LizardGPU_offsetsFromSizes is the host form of the prefix sum (offsets[nBlocks] = total). */
void LizardGPU_shardRange(size_t nBlocks, int rank, int nRanks, size_t* first, size_t* count);
void LizardGPU_offsetsFromSizes(const uint32_t* sizes, size_t nBlocks, uint64_t* offsets);
int  LizardGPU_compressBlocks_sharded(int nDevices, const int* devices, const void* const* d_src, size_t nBlocks,
                                      size_t blockSize, size_t lastBlockSize, void* const* d_dst, size_t dstStride,
                                      uint32_t* const* d_allSizes, uint64_t* const* d_offsets, int level);
int  LizardGPU_commUniqueId(void* id128);
int  LizardGPU_commInitRank(const void* id128, int nRanks, int rank);
int  LizardGPU_gatherSizes_device(const uint32_t* d_localSizes, size_t nBlocks, uint32_t* d_allSizes,
                                  uint64_t* d_offsets, void* stream);
int  LizardGPU_commDestroy(void);
/* The transport of the size exchange is a table of four calls (u32 elements; `comm` and `stream` are passed through as the
 * library received them; allGather is in place when send == recv + rank*count, as ncclAllGather; every call returns 0 or a
 * negative LIZARDGPU_ERR_*).  RCCL fills it by default — resolved from a copy the process has already mapped (torch's in a
 * torchrun job) before librccl.so.1 is loaded, LizardGPU_rcclShared() = 1 / 0 / -1 (not resolved yet).  LizardGPU_setCollectives
 * installs another transport (NULL: back to RCCL; a table with a NULL member is refused); with one installed NO RCCL is involved:
 * LizardGPU_compressBlocks_sharded and LizardGPU_gatherSizes_device pass the rank index as `comm`, and LizardGPU_commInitRank only
 * records rank and rank count (its id argument is ignored).  The exchange logic itself (lizard_amd/csrc/lizard_shard_core.h) is transport-agnostic:
 * tests/shard_fake.cpp runs it with 2 and 3 ranks over shared memory on a CPU. */
typedef struct {
    int (*allGather)(const void* send, void* recv, size_t count, void* comm, void* stream);
    int (*broadcast)(const void* send, void* recv, size_t count, int root, void* comm, void* stream);
    int (*groupStart)(void);
    int (*groupEnd)(void);
} LizardGPU_Collectives;
int  LizardGPU_setCollectives(const LizardGPU_Collectives* table);
int  LizardGPU_rcclShared(void);
/* What carries the size exchange of this process, as the transport itself reports it — a figure measured over N ranks can say
 * whether RCCL saw N ranks.  LizardGPU_commInitRank and the communicators of LizardGPU_compressBlocks_sharded are checked against
 * ncclCommCount / ncclCommUserRank when they are made (a mismatch fails the call with -LIZARDGPU_ERR_RCCL).
 *   info[0]  0 = RCCL, 1 = a table installed with LizardGPU_setCollectives
 *   info[1]  ranks the caller asked for in LizardGPU_commInitRank (0 = no rank communicator)
 *   info[2]  ranks the RCCL rank communicator reports (ncclCommCount; 0 = none, -1 = this RCCL does not export the call)
 *   info[3]  this process's rank as RCCL reports it (ncclCommUserRank; -1 = n/a)
 *   info[4]  ncclGetVersion (0 = RCCL not loaded)
 *   info[5]  ranks of the single-process communicators of LizardGPU_compressBlocks_sharded (0 = none)
 * Always returns 0. */
int  LizardGPU_commInfo(int info[6]);

/* ---- decompression ----
 * Independent blocks as Lizard_decompress_safe() decodes them (reference lib/lizard_decompress.h:64, lizard_decompress.c:267;
 * no dictionary, no prefix): every level's container, huff0 streams, fastLZ4 and LIZv1 codewords.  One wave per block.
 * _device: block i is d_srcSizes[i] bytes at d_src + i*srcStride (the layout LizardGPU_compressBlocks_device leaves behind)
 * and is decoded to d_dst + i*dstStride (capacity dstStride); d_outSizes[i] = decoded size, 0xFFFFFFFF if the block is
 * corrupt or does not fit.  Enqueued on `stream`.  _host: block i is src[offsets[i] .. offsets[i+1]) (the layout of
 * LizardGPU_compressBlocks_host_packed); synchronous.  LizardGPU_decompress_safe is the one-block twin of
 * Lizard_decompress_safe: decoded size, or a negative value for a corrupt block / maxDecompressedSize too small.
 * Memory-safe on any input: never reads outside a compressed block, never writes outside a block's output slot. */
int LizardGPU_decompressBlocks_device(const void* d_src, size_t srcStride, const uint32_t* d_srcSizes, size_t nBlocks,
                                      void* d_dst, size_t dstStride, uint32_t* d_outSizes, void* stream);
int LizardGPU_decompressBlocks_host(const void* src, const uint64_t* offsets, size_t nBlocks, void* dst, size_t dstStride,
                                    uint32_t* outSizes);
int LizardGPU_decompress_safe(const char* source, char* dest, int compressedSize, int maxDecompressedSize);


/* Kernel-only duration of the most recent LizardGPU_compressBlocks_* call on the selected device, measured with HIP
 * events on the launch stream, in milliseconds (blocks until that launch finished; host-buffer calls: the sum over
 * their chunks). < 0 if unavailable. */
float LizardGPU_lastKernelMs(void);

/* Number of resident waves (= blocks compressed concurrently) the launcher uses on this device. */
int LizardGPU_residentWaves(void);

/* Launches on different streams.  A launch needs a scratch arena (2.6 GiB), a block counter and — levels 11/31, 20/40, 21/41,
 * 22/42 — per-wave tables to itself.  Launches that fill the machine, the hashChain levels and decompression share the context's own and
 * run one after the other (the second waits on the device for the first); a compress launch SMALLER than the machine that arrives
 * on another stream while that arena is busy gets one of up to three more, allocated on first need, and runs beside it on the CUs
 * it leaves free.  LIZARDGPU_ARENAS=1..4 caps the total (default 4; 1 = every launch waits for the previous one).
 * Returns how many exist right now on the selected device (>= 1 once it was used; 0 before / without a device). */
int LizardGPU_arenasInUse(void);

/* Device memory.  A context (one per device) keeps a scratch arena (one slot per resident wave: 2.7 GB on a 256-CU device), and
 * allocates on first use: up to three more arenas for small launches on concurrent streams (released again after 64 launches that
 * did not need them), per-wave tables (levels 20/40/21/41: 256 MiB; 11/31/22/42: 4 GiB), hashChain work areas (levels 12-17 / 32-38: up
 * to half of the free memory, at most 128 GiB), and the staging of the host-buffer entries (three chunks of 256 MiB in flight).
 * LizardGPU_setMemoryBudget(bytes) bounds the sum per device (0 = no bound, the default): tables and work areas then get fewer
 * slots than there are resident waves (fewer blocks in flight: slower, same bytes), what another level left behind is given up
 * first, extra arenas are only made when they fit, host-buffer chunks shrink to bytes / 64; an allocation that still does not fit
 * fails its call with -LIZARDGPU_ERR_NOMEM (Lizard_compress*: 0).  The call releases what every context holds (like
 * LizardGPU_shutdown, communicators excepted) — set it before first use or between uses, not under load; below one scratch arena
 * + 256 MiB it is refused (-LIZARDGPU_ERR_ARG, LizardGPU_lastError names the minimum).  The environment knobs stay
 * (LIZARDGPU_ARENAS, LIZARDGPU_HC_WORKAREA_MB, LIZARDGPU_CHUNK_MB).
 * LizardGPU_memoryInUse: bytes the selected device's context holds in those buffers.  LizardGPU_trim: gives back everything but the
 * context's own scratch arena on the selected device (waits for the device to be idle). */
int    LizardGPU_setMemoryBudget(size_t bytes);
size_t LizardGPU_memoryBudget(void);
size_t LizardGPU_memoryInUse(void);
int    LizardGPU_trim(void);

/* Calls of this process that could not compress on the GPU (level without a kernel, no device, HIP failure) and therefore returned
 * 0 (Lizard_compress*) or stored their blocks raw (LizardF_compress*, non-strict): every one is counted here, and the 1st, 2nd,
 * 4th, 8th ... prints one line on stderr with the reason.  The strict twins (LizardGPU_compressFrame ...) return an error instead. */
unsigned long long LizardGPU_degradedCalls(void);

/* The one-block entry points of part 1 (Lizard_compress, _extState, _continue) are COMBINED: callers that arrive while a launch is
 * in flight leave together in the next one — one ragged batch, one block per CU — instead of queueing behind a lock, so N host
 * threads compress N blocks per launch (lizard_amd/csrc/lizard_pipeline_host.c).  Launches made / blocks carried so far on the
 * selected device (either pointer may be NULL); 0 or -LIZARDGPU_ERR_*. */
int LizardGPU_combinerStats(unsigned long long* batches, unsigned long long* blocks);
/* Tuning aid: where the batches' time went, seconds since the process started — [0] waiting for the device context, [1] the
 * members' copy-in, [2] the GPU part (H2D, kernel, compaction, D2H), [3] until the last member had copied out. */
int LizardGPU_combinerProfile(double out[4]);

/* =====================================================================================================
 * Part 3 — frame production on the batched GPU path.
 *
 * A twin of the reference's frame COMPRESSOR: LizardGPU_compressBegin / _compressUpdate / _flush / _compressEnd
 * follow lib/lizard_frame.c:362-424, :501-599, :610-637, :651-677 call for call, and LizardGPU_compressFrame is built
 * on them like LizardF_compressFrame (lizard_frame.c:260-316).  They write byte for byte what the reference writes for
 * the same preferences and the same sequence of calls in independent-block mode (reference built with
 * -DLIZARD_RESET_MEM, the zero-state oracle): frame header, LE32-sized block records (bit 31 = stored raw), end
 * mark, XXH32 content checksum.  Every run of blocks an Update call covers is ONE batch through the block kernels,
 * and the block records are assembled on the device (prefix sum of sizes + compaction), so only the frame body
 * crosses PCIe, once.  The content checksum runs on a host thread beside the GPU work.
 * The reference keeps frame compression and decompression in ONE object (lizard_frame.c), so these symbols are
 * prefixed LizardGPU_ and coexist with a linked reference LizardF_* (INTEGRATION.md §2).
 *
 * LizardGPU_framePrefs_t is layout-identical to LizardF_preferences_t (lib/lizard_frame.h:111-125): a caller
 * holding the reference type passes (const LizardGPU_framePrefs_t*)&prefs.
 * Size_t results: bytes written, or an error code that LizardGPU_frameIsError() recognises; codes are the
 * reference's (size_t)-LizardF_ERROR_* values (lib/lizard_frame_static.h:57-67).  Refused, never emulated:
 * linked-block frames larger than one block (blockMode_invalid), levels without a GPU kernel
 * (compressionLevel_invalid) and skippable frames (frameType_unknown).
 * ===================================================================================================== */
typedef LizardF_frameInfo_t   LizardGPU_frameInfo_t;
typedef LizardF_preferences_t LizardGPU_framePrefs_t;

enum {                                       /* LizardF_errorCodes, lib/lizard_frame_static.h:57-67 */
    LIZARDGPU_FRAME_ERR_GENERIC = 1, LIZARDGPU_FRAME_ERR_maxBlockSize_invalid = 2, LIZARDGPU_FRAME_ERR_blockMode_invalid = 3,
    LIZARDGPU_FRAME_ERR_compressionLevel_invalid = 5, LIZARDGPU_FRAME_ERR_headerVersion_wrong = 6,
    LIZARDGPU_FRAME_ERR_blockChecksum_unsupported = 7, LIZARDGPU_FRAME_ERR_reservedFlag_set = 8, LIZARDGPU_FRAME_ERR_allocation_failed = 9,
    LIZARDGPU_FRAME_ERR_dstMaxSize_tooSmall = 11, LIZARDGPU_FRAME_ERR_frameHeader_incomplete = 12, LIZARDGPU_FRAME_ERR_frameType_unknown = 13,
    LIZARDGPU_FRAME_ERR_frameSize_wrong = 14, LIZARDGPU_FRAME_ERR_decompressionFailed = 16, LIZARDGPU_FRAME_ERR_headerChecksum_invalid = 17,
    LIZARDGPU_FRAME_ERR_contentChecksum_invalid = 18, LIZARDGPU_FRAME_ERR_maxCode = 19
};

/* replaces LizardF_isError, lib/lizard_frame.h:59 / lizard_frame.c:179 */
unsigned LizardGPU_frameIsError(size_t code);
/* replaces LizardF_compressFrameBound, lib/lizard_frame.h:122 / lizard_frame.c:229 (same value).
 * KNOWN SHORTFALL, inherited with the value: the bound counts a last block of ONE byte as one byte of payload, but such a block
 * makes a record with 6 bytes of payload.  A header without content size is 8 bytes shorter than the 15 the bound allows for, which
 * hides the 5 missing bytes; with a content size nothing hides them, and a source of 1 byte, or of k * block size + 1 bytes whose
 * last block is stored as that record, is answered dstMaxSize_tooSmall by every compress entry of Parts 1c and 3 when dst has
 * exactly the bound.  Give such a frame the bound + 5 bytes (api.compress_stream_device gives every frame 8). */
size_t LizardGPU_compressFrameBound(size_t srcSize, const LizardGPU_framePrefs_t* preferencesPtr);
/* replaces LizardF_compressFrame, lib/lizard_frame.h:134 / lizard_frame.c:260 (host buffers, synchronous) */
size_t LizardGPU_compressFrame(void* dstBuffer, size_t dstMaxSize, const void* srcBuffer, size_t srcSize,
                               const LizardGPU_framePrefs_t* preferencesPtr);

/* ---- the same frame for data that already lies in DEVICE memory, written into device memory ----
 * d_src (srcSize bytes) and d_dst (dstCapacity bytes) are device pointers.  The call answers exactly what LizardGPU_compressFrame
 * answers for the same source bytes, preferences and capacity: the same return value (a size or an error code) and the same frame
 * bytes — the refusals above and maxBlockSize_invalid, dstMaxSize_tooSmall below LizardGPU_compressFrameBound, the level clamp, the
 * block size id shrunk to the input, contentSize != 0 meaning "write srcSize", srcSize == 0.  Like its twin it answers
 * dstMaxSize_tooSmall for the one frame that can exceed a buffer of exactly the bound: a 1-byte last block (a 10-byte record where the
 * bound counted 5) behind blocks that were all stored raw, under a header that carries the content size.
 * SYNCHRONOUS, like LizardGPU_decompressFrame_device: the work is ordered after what `stream` holds at the call, and when the call
 * returns the frame is visible to work enqueued on `stream` afterwards.  Nothing outside d_dst[0..dstCapacity) is written, nothing
 * outside d_src[0..srcSize) is read; the bytes of d_dst behind the returned size are unspecified, and so is d_dst after an error
 * (below the bound it is left untouched).
 * The input is compressed in chunks of whole blocks (LIZARDGPU_CHUNK_MB; LIZARDGPU_FRAME_CHUNK_BLOCKS = 1 .. 2^20 overrides the blocks
 * per chunk, read at every call) into the context's staging slots, and the block records are moved to their place in d_dst on the
 * device; where a chunk's records start is kept in device memory, so all chunks are enqueued without a host round trip.  Without a
 * content checksum no payload byte crosses PCIe in either direction.  With one, XXH32 runs on the HOST: the source is copied to
 * pinned memory once, in pieces, and hashed by the calling thread while the device compresses — the call is then bounded by one host
 * thread's hashing rate.
 * No device or a HIP failure is LIZARDGPU_FRAME_ERR_GENERIC (LizardGPU_lastError has the text): never a host fall-back, never blocks
 * stored raw instead. */
size_t LizardGPU_compressFrame_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize,
                                      const LizardGPU_framePrefs_t* preferencesPtr, void* stream);
/* Since process start, selected device: [0] blocks whose compressed form went into a frame, [1] blocks stored raw, [2] chunks
 * launched, [3] source bytes copied to the host for the checksum.  0 or -LIZARDGPU_ERR_*. */
int    LizardGPU_frameCompressDeviceStats(unsigned long long out[4]);

/* ---- many buffers in device memory, one frame each, in ONE batch ----
 * d_dsts, dstCapacities, d_srcs, srcSizes and results are HOST arrays of nFrames entries; the pointers they hold are device pointers
 * on the selected device.  Per frame i, results[i] and the bytes d_dsts[i][0 .. results[i]) are what
 * LizardGPU_compressFrame_device(d_dsts[i], dstCapacities[i], d_srcs[i], srcSizes[i], preferencesPtr, stream) answers — and so, by
 * that function's contract, what LizardGPU_compressFrame answers: its refusals in its order, GENERIC for a null pointer in a frame's
 * entry, the level clamp, the block size id shrunk to EACH frame's own input (frames of one batch may have different block sizes and
 * header bytes), contentSize != 0 meaning "write this frame's srcSize", srcSize == 0, dstMaxSize_tooSmall for the 1-byte last block at
 * exactly the bound.  A refused frame does not stop the others; one refused up front (everything but that last case) leaves its d_dst
 * untouched.  Nothing outside d_dsts[i][0 .. dstCapacities[i]) is written, nothing outside d_srcs[i][0 .. srcSizes[i]) is read;
 * sources may start at any byte address.  Destinations that overlap each other or a source are the caller's error.
 * Returns 0 once every results[i] has been decided this way (LizardGPU_lastError names the first refused frame, if any);
 * -LIZARDGPU_ERR_ARG for a null array with nFrames > 0; -LIZARDGPU_ERR_* when the machinery fails (no device, HIP, allocation:
 * LizardGPU_lastError has the text), and then every frame not already refused gets LIZARDGPU_FRAME_ERR_GENERIC.  nFrames == 0
 * returns 0 and touches nothing.  Never a host fall-back, never blocks stored raw instead.
 * SYNCHRONOUS like its single-frame sibling: ordered after what `stream` holds at the call; on return all frames are visible to work
 * enqueued on `stream` afterwards.
 * The blocks of all frames form one list that is compressed in chunks (LIZARDGPU_CHUNK_MB over the batch's largest block size;
 * LIZARDGPU_FRAME_CHUNK_BLOCKS as above), so a batch of small buffers fills the device as one large buffer does, and the host waits
 * once per call.  NO payload byte crosses PCIe in either direction, checksum or not: what crosses is a table entry per frame and per
 * block going up and a result record per frame coming down.  The content checksums are computed on the device, all frames side by
 * side; ONE frame's XXH32 is serial, so a batch cannot finish before its largest frame is hashed, at a per-frame rate that is not
 * measured yet and certainly below a host core's — one huge buffer with a checksum belongs with LizardGPU_compressFrame_device.
 * LizardGPU_frameCompressDeviceStats counts this entry's blocks and chunks in [0], [1], [2]; it never adds to [3]. */
int    LizardGPU_compressFrames_device(size_t nFrames, void* const* d_dsts, const size_t* dstCapacities, const void* const* d_srcs,
                                       const size_t* srcSizes, size_t* results, const LizardGPU_framePrefs_t* preferencesPtr, void* stream);

/* ---- many buffers in device memory, one frame each, BACK TO BACK in one device buffer: a .liz stream written in one call ----
 * The writing half of LizardGPU_decompressStream_device.  d_srcs, srcSizes, prefixes, prefixSizes and frameOffsets are HOST arrays;
 * d_srcs[i] and d_dst are device pointers on the selected device, prefixes[i] points to prefixSizes[i] bytes in HOST memory
 * (prefixes == prefixSizes == NULL: no prefixes).  d_dst[0 .. returned size) is, for i = 0 .. nFrames - 1, prefixes[i][0 ..
 * prefixSizes[i]) followed by frame i.  A prefix is opaque to this entry: a tensor stream passes its skippable tensor headers.
 * Frame i is byte for byte what LizardGPU_compressFrame_device writes for d_srcs[i], srcSizes[i], the same prefs and a capacity of
 * LizardGPU_compressFrameBound(srcSizes[i], prefs) + 8: the level clamp, the block size id shrunk to EACH frame's own input,
 * contentSize != 0 meaning "write this frame's srcSize", srcSize == 0, a 1-byte last block.  frameOffsets (may be NULL, else
 * nFrames + 1 entries): frameOffsets[i] is where prefix i starts, frameOffsets[nFrames] the returned size.
 * Returns the stream's size or a code LizardGPU_frameIsError recognises:
 *   - a frame the single-frame entry would refuse up front (level without a kernel, linked mode above one block, skippable frame
 *     type, block size id out of range, a null source with a non-zero size, a null prefix with a non-zero size) is refused BEFORE
 *     anything is launched: that frame's code, *failedFrame (may be NULL) its index, d_dst untouched.  The first such frame in index
 *     order decides: a stream with a hole is not a stream.
 *   - dstMaxSize_tooSmall when the stream does not fit dstCapacity; nothing outside d_dst[0 .. dstCapacity) is written, and what
 *     d_dst holds is unspecified.  LizardGPU_compressStreamBound bytes never get this answer: that is the sum of the prefix sizes and
 *     of every frame's LizardGPU_compressFrameBound + 8, so the bound's known 5-byte shortfall is covered.
 *   - GENERIC for a null array with nFrames > 0, for 2^32 blocks or more, and when the machinery fails (no device, HIP, allocation);
 *     LizardGPU_lastError has the text.  Never a host fall-back.
 * nFrames == 0 returns 0 and touches nothing.  Nothing outside d_srcs[i][0 .. srcSizes[i]) is read; sources may start at any byte
 * address.  SYNCHRONOUS like its siblings: ordered after what `stream` holds at the call; on return the stream is visible to work
 * enqueued on `stream` afterwards.
 * The blocks of all frames form one list that is compressed in chunks as in LizardGPU_compressFrames_device (the same
 * LIZARDGPU_FRAME_CHUNK_BLOCKS); where a record goes is the host's sum of everything in front of it that does not depend on
 * compressed sizes plus a prefix sum of record sizes that the device carries from chunk to chunk, so the host waits once per call.
 * NO payload byte crosses PCIe: the tables and the prefix bytes go up in one copy, 16 bytes (and the offsets, when asked for) come
 * down.  The content checksums are computed on the device as in LizardGPU_compressFrames_device.
 * LizardGPU_streamCompressDeviceStats, since process start, selected device: [0] frames written, [1] blocks stored raw, [2] chunks
 * launched, [3] calls that launched anything.  This entry adds nothing to LizardGPU_frameCompressDeviceStats. */
size_t LizardGPU_compressStreamBound(size_t nFrames, const size_t* srcSizes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs);
size_t LizardGPU_compressStream_device(void* d_dst, size_t dstCapacity, size_t nFrames, const void* const* d_srcs, const size_t* srcSizes,
                                       const void* const* prefixes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs,
                                       uint64_t* frameOffsets, size_t* failedFrame, void* stream);
int    LizardGPU_streamCompressDeviceStats(unsigned long long out[4]);

/* Streaming form.  LizardGPU_cctx_t replaces LizardF_compressionContext_t (lib/lizard_frame.h:145); the functions
 * replace LizardF_createCompressionContext / _freeCompressionContext (:157-158, int result: 0 or -LIZARDGPU_FRAME_ERR_*),
 * LizardF_compressBegin (:169), LizardF_compressBound (:178), LizardF_compressUpdate (:190), LizardF_flush (:202) and
 * LizardF_compressEnd (:213).  The reference's LizardF_compressOptions_t only carries stableSrc, which matters to
 * linked blocks alone, so the argument is dropped. */
typedef struct LizardF_cctx_s LizardGPU_cctx_t;      /* the object LizardF_createCompressionContext makes, in its strict mode */
int    LizardGPU_createCompressionContext(LizardGPU_cctx_t** cctxPtr);
int    LizardGPU_freeCompressionContext(LizardGPU_cctx_t* cctx);
size_t LizardGPU_compressBegin(LizardGPU_cctx_t* cctx, void* dstBuffer, size_t dstMaxSize, const LizardGPU_framePrefs_t* preferencesPtr);
size_t LizardGPU_compressBound(size_t srcSize, const LizardGPU_framePrefs_t* preferencesPtr);
size_t LizardGPU_compressUpdate(LizardGPU_cctx_t* cctx, void* dstBuffer, size_t dstMaxSize, const void* srcBuffer, size_t srcSize);
size_t LizardGPU_flush(LizardGPU_cctx_t* cctx, void* dstBuffer, size_t dstMaxSize);
size_t LizardGPU_compressEnd(LizardGPU_cctx_t* cctx, void* dstBuffer, size_t dstMaxSize);

/* =====================================================================================================
 * Part 3b — whole frames decoded on the GPU.
 *
 * LizardF_decompress (Part 1c) stays what it is: streaming, any segmentation, one host thread.  These entries take ONE whole
 * frame in host memory and decode every block that can be decoded on its own on the device, in batches: the host walks the
 * header and the chain of block records, chunks of whole records go through pinned staging to lz_unframe_kernel (one wave per
 * record: stored-raw records are copied, compressed ones decoded), up to three chunks in flight, and the calling thread finishes
 * the chunks in order (copy to dst, content checksum).  A block of a LINKED frame that copies from before its own start is
 * recognised exactly by the kernel and decoded on the host behind the bytes that are final by then; a linked frame in which most
 * blocks do so (the reference's linked frames; never this library's, Part 1) is handed to the host decoder after its first chunk.
 * The result is what LizardF_decompress produces for the same bytes; for damaged input the same refusals with the same codes for
 * header, content-checksum, frame-size errors (a corrupt block: decompressionFailed in a linked frame, GENERIC in an independent one).
 * Strict like Part 3: no device or a HIP failure is LIZARDGPU_FRAME_ERR_GENERIC (LizardGPU_lastError has the text), never a
 * silent host decode.
 * ===================================================================================================== */

/* Decodes the ONE frame that starts at src.  Returns the bytes written to dst, or a code LizardGPU_frameIsError() recognises.
 * *srcConsumedPtr (may be NULL) = bytes of src the frame occupied (0 on error): a caller walks concatenated frames by calling
 * again (for frames in device memory LizardGPU_decompressStream_device does it in batches).  A skippable frame decodes to 0
 * bytes.  dst too small for the frame: dstMaxSize_tooSmall; nothing outside dst[0..dstCapacity) is ever written.  A frame that
 * ends before its end mark / checksum (LizardF_decompress would ask for more input): frameHeader_incomplete when src ends inside
 * the header, GENERIC behind it. */
size_t LizardGPU_decompressFrame(void* dst, size_t dstCapacity, const void* src, size_t srcSize, size_t* srcConsumedPtr);

/* Upper bound of what the frame at src decodes to, without decoding: the sum over its block records of (stored raw ? record size
 * : the frame's maximum block size), or the header's content size when it carries one that is smaller (for every frame
 * LizardF_decompress accepts that is the exact size).  Error code as LizardGPU_decompressFrame for a header / record chain that
 * is refused or ends early.  Pure host code. */
size_t LizardGPU_decompressFrameBound(const void* src, size_t srcSize);

/* The record table the decoder works from (pure host code, no device needed): for record i the byte offset in src of its payload
 * (behind the LE32 word) and the word itself (bit 31 = stored raw).  Fills at most maxRecords entries (the arrays may be NULL),
 * *nRecords = how many the frame has, *frameBytes = header + records + end mark + checksum; info (may be NULL) = the header's
 * fields.  0 or -LIZARDGPU_FRAME_ERR_*. */
int LizardGPU_frameIndex(const void* src, size_t srcSize, LizardGPU_frameInfo_t* info, uint64_t* payloadOffsets,
                         uint32_t* recordWords, size_t maxRecords, size_t* nRecords, size_t* frameBytes);

/* Since process start, selected device: [0] blocks decoded by the kernel, [1] raw records copied by the kernel, [2] blocks decoded
 * again on the host because they reach into their history, [3] frames whose remainder was handed to the host decoder.
 * 0 or -LIZARDGPU_ERR_*.  LizardGPU_frameDecodePackedChunks: chunks that had a short block in the middle and were packed on the
 * device before the copy. */
int LizardGPU_frameDecodeStats(unsigned long long out[4]);
unsigned long long LizardGPU_frameDecodePackedChunks(void);

/* ---- the same for a frame that already lies in DEVICE memory, decoded into device memory ----
 * Nothing but a few bytes per record crosses PCIe: the frame is walked on the device (one wave, in segments of 4 096 records,
 * LIZARDGPU_WALK_RECORDS overrides; the walk of a segment runs while the segment before it is decoded) and every record is decoded
 * straight to its place in d_dst.  Records behind a short block in the middle of a frame (flushed frames) go through the context's
 * staging slots and are moved into place on the device. */

#define LIZARDGPU_FRAME_SKIP_CHECKSUM 1u   /* do not verify the content checksum (it is still required to be present) */

/* Decodes the ONE frame that starts at d_src (device memory, srcSize bytes) into d_dst (device memory).  SYNCHRONOUS: the work
 * is ordered after what `stream` holds at the call, and when the call returns the result is visible to work enqueued on `stream`
 * afterwards.  Return value, *srcConsumedPtr (a host value, may be NULL) and the decoded bytes are what LizardGPU_decompressFrame
 * answers for the same frame bytes in host memory, for every input, intact or damaged, and every capacity — including the order of
 * its refusals: a record chain that is refused outranks a corrupt block or a buffer that is too small.  Nothing outside
 * d_dst[0..dstCapacity) is written, nothing outside d_src[0..srcSize) is read; the bytes of d_dst behind the returned size are
 * unspecified.  A skippable frame decodes to 0 bytes.
 * Content checksum: XXH32 is one serial chain over the whole stream and runs on the HOST.  Unless flags has
 * LIZARDGPU_FRAME_SKIP_CHECKSUM, the decoded bytes of a frame that carries a checksum are copied to pinned host memory in pieces
 * and hashed there by the calling thread — a segment's bytes while the next segment decodes, the last or only segment's after its
 * decode: that costs one D2H crossing and bounds the call by the host's hashing rate.  With
 * the flag a wrong stored checksum is not noticed; a frame too short to hold its checksum is refused either way.
 * A LINKED frame with a block that reaches into its history (the reference's linked frames, never this library's) is finished on
 * the host: the frame is copied to pinned memory, decoded by LizardGPU_decompressFrame and the result copied into d_dst.
 * No device or a HIP failure is LIZARDGPU_FRAME_ERR_GENERIC (LizardGPU_lastError has the text), never a silent fall-back. */
size_t LizardGPU_decompressFrame_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr,
                                        unsigned flags, void* stream);

/* LizardGPU_frameIndex for a frame in device memory, walked on the device: d_payloadOffsets / d_recordWords are DEVICE arrays of
 * maxRecords entries (either may be NULL); info, *nRecords and *frameBytes are host values.  The same return code and values as
 * LizardGPU_frameIndex for the same bytes.  Synchronous, ordered after what `stream` holds. */
int LizardGPU_frameIndex_device(const void* d_src, size_t srcSize, LizardGPU_frameInfo_t* info, uint64_t* d_payloadOffsets,
                                uint32_t* d_recordWords, size_t maxRecords, size_t* nRecords, size_t* frameBytes, void* stream);

/* Since process start, selected device: [0] records decoded straight into the caller's buffer, [1] records that went through
 * staging and were gathered into place, [2] frames finished on the host because a block needed its history, [3] walk segments
 * launched.  0 or -LIZARDGPU_ERR_*. */
int LizardGPU_frameDecodeDeviceStats(unsigned long long out[4]);

/* Records per walk segment in effect (LIZARDGPU_WALK_RECORDS when it holds 1 .. 2^20, else the default), and the maximum block
 * size of a frame's block size id (0 = the default id; 0 for an id above 7). */
size_t LizardGPU_frameWalkRecords(void);
size_t LizardGPU_frameBlockSize(unsigned blockSizeID);

/* ---- MANY frames in device memory, each decoded into its own device buffer, in ONE batch ----
 * The reading half of LizardGPU_compressFrames_device: a state_dict, cache pages, a list of activations.  Frame i lies at d_srcs[i]
 * (srcSizes[i] bytes) and decodes into d_dsts[i] (dstCapacities[i] bytes); d_dsts, dstCapacities, d_srcs, srcSizes, results and
 * srcConsumed (may be NULL) are HOST arrays of nFrames entries.  results[i], srcConsumed[i] and the bytes d_dsts[i][0 .. results[i])
 * are what LizardGPU_decompressFrame_device(d_dsts[i], dstCapacities[i], d_srcs[i], srcSizes[i], &used, flags, stream) answers — and
 * so, by that function's contract, what LizardGPU_decompressFrame answers for the same bytes: intact and damaged frames, every
 * capacity, LIZARDGPU_FRAME_SKIP_CHECKSUM honoured, a skippable frame decodes to 0 bytes.  A null pointer in an entry with a non-zero
 * size is LIZARDGPU_FRAME_ERR_GENERIC for that frame only; a refused frame does not stop the others.  Nothing outside
 * d_dsts[i][0 .. dstCapacities[i]) is written, nothing outside d_srcs[i][0 .. srcSizes[i]) is read; sources and destinations may start
 * at any byte address.  Overlapping destinations are the caller's error; several entries may share a source.
 * The host waits TWICE per call, however many frames: every frame is walked on the device side by side (one wave each) to count its
 * records; then the walk that fills the record tables, ONE decode launch over all records of all frames (each in place in its frame's
 * buffer), the per-frame settling, the content checksums — XXH32 of the decoded bytes ON THE DEVICE, sixteen frames per wave — and the
 * comparison with the stored ones are enqueued together.  No payload byte crosses PCIe, checksum or not.
 * The device settles the frames LizardGPU_compressFrames_device writes (every record but the last fills the frame's block size).  A
 * frame the walk accepts that is anything else — a short record in the middle (flushed frames), a block that fails or needs its
 * history (the reference's linked frames), a buffer that is too small, a wrong content size or checksum — is handed to
 * LizardGPU_decompressFrame_device after the batch part, one call each; [2] of the statistics counts them.
 * Returns 0 once every results[i] has been decided (LizardGPU_lastError names the first refused frame); -LIZARDGPU_ERR_ARG for a null
 * array with nFrames > 0, or when nFrames or the batch's record count is 2^32 or more; -LIZARDGPU_ERR_* when the machinery fails:
 * every frame not yet decided then answers LIZARDGPU_FRAME_ERR_GENERIC with 0 bytes consumed.  nFrames == 0 returns 0 and touches
 * nothing.  SYNCHRONOUS and ordered after what `stream` holds, like LizardGPU_decompressFrame_device.  Never a host fall-back for a
 * frame of this library. */
int LizardGPU_decompressFrames_device(size_t nFrames, void* const* d_dsts, const size_t* dstCapacities, const void* const* d_srcs,
                                      const size_t* srcSizes, size_t* results, size_t* srcConsumed, unsigned flags, void* stream);

/* LizardGPU_frameIndex_device without tables for nFrames frames, in one launch and one host wait: codes[i] is what that function
 * returns for frame i, infos[i] is filled exactly where it fills *info, nRecords[i] / frameBytes[i] are its values (0 for a refused
 * frame).  Any of the four output arrays (host arrays) may be NULL.  0, or -LIZARDGPU_ERR_* (null input array, 2^32 frames or more,
 * a failure of the machinery: every codes[i] is -LIZARDGPU_FRAME_ERR_GENERIC then). */
int LizardGPU_framesInfo_device(size_t nFrames, const void* const* d_srcs, const size_t* srcSizes, LizardGPU_frameInfo_t* infos,
                                size_t* nRecords, size_t* frameBytes, int* codes, void* stream);

/* LizardGPU_decompressFrames_device since process start, selected device: [0] records decoded by the batch kernel, [1] frames
 * settled on the device, [2] frames handed to LizardGPU_decompressFrame_device, [3] batch calls that launched anything.
 * 0 or -LIZARDGPU_ERR_*. */
int LizardGPU_framesDecodeDeviceStats(unsigned long long out[4]);

/* ---- a STREAM of frames in device memory — back to back in one buffer, no table of pointers — decoded into one device buffer ----
 * What a .liz file is when frames were appended, what `lizard -d` reads, and what a saved state_dict or a file of cache pages is once
 * it has been loaded into device memory.  The contract is this loop: pos = 0, out = 0; while pos < srcSize, call
 * LizardGPU_decompressFrame_device(d_dst + out, dstCapacity - out, d_src + pos, srcSize - pos, &used, flags, stream); on an error code
 * stop; otherwise out += result, pos += used, frames += 1.  The entry answers what the loop answers: the return value is out, or the
 * first error code; *srcConsumedPtr = pos (on error: the offset of the frame that was refused), *nFramesPtr = the frames completed,
 * *decodedPtr = out (on error the bytes d_dst[0 .. out) of the completed frames are valid); any of the three may be NULL.
 * srcSize == 0 returns 0 and touches nothing.  A skippable frame counts as a frame of 0 bytes; LIZARDGPU_FRAME_SKIP_CHECKSUM is
 * honoured.  SYNCHRONOUS and ordered after what `stream` holds; nothing outside d_src[0 .. srcSize) is read, nothing outside
 * d_dst[0 .. dstCapacity) is written.  Strict like the rest of Part 3b: no device or a HIP failure is LIZARDGPU_FRAME_ERR_GENERIC
 * (LizardGPU_lastError has the text).
 * How: one wave follows the chain of frames on the device (the next frame starts where this one ends: the chain is serial, and no
 * boundary is ever guessed) in segments of 4 096 frames (LIZARDGPU_STREAM_WALK_FRAMES = 1 .. 2^20 overrides; read at every call),
 * one host wait per segment that succeeds.  A frame's place in d_dst is the sum of the decoded sizes in front of it, and the header gives a size
 * when it carries a content size, when the frame is skippable or when it has no records: the longest run of frames in which every
 * frame but the last has such a size is ONE batch through LizardGPU_decompressFrames_device (two more waits), every frame with its
 * size as its capacity, the last with the real remainder.  The first frame of the stream that its batch does not answer with exactly
 * its header's size (a refused frame, a chain the walk refuses, a linked frame of several records) is handed to
 * LizardGPU_decompressFrame_device with the loop's own arguments, and an error there is the call's answer.
 * A stream of frames WITH content sizes is one batch, however many frames.  A stream of N frames WITHOUT content sizes is N batches of
 * one frame: correct, and no faster than the loop.  (The reference's CLI writes no content size by default; its files are normally
 * one frame, which is one batch.) */
size_t LizardGPU_decompressStream_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr,
                                         size_t* nFramesPtr, size_t* decodedPtr, unsigned flags, void* stream);

/* The stream walk alone.  For frame k of the stream: its offset, its length, the header's fields and its record count, in HOST arrays
 * of maxFrames entries (any of the four may be NULL; entries behind maxFrames are not written).  *nFrames = the frames the stream has,
 * *streamBytes = the bytes they occupy.  0, or -LIZARDGPU_FRAME_ERR_* of the first frame whose chain is refused: *nFrames is the number
 * of frames in front of it then and *streamBytes its offset (infos[*nFrames] is filled where LizardGPU_frameIndex_device fills *info).
 * The per-frame values are those of LizardGPU_frameIndex_device called on each frame.  No device or a HIP failure:
 * -LIZARDGPU_FRAME_ERR_GENERIC.  Synchronous, ordered after what `stream` holds. */
int LizardGPU_streamIndex_device(const void* d_src, size_t srcSize, uint64_t* frameOffsets, uint64_t* frameBytes, LizardGPU_frameInfo_t* infos,
                                 size_t* nRecords, size_t maxFrames, size_t* nFrames, size_t* streamBytes, void* stream);

/* LizardGPU_decompressStream_device / LizardGPU_streamIndex_device since process start, selected device: [0] frames answered by a
 * batch, [1] batches launched, [2] frames this entry handed to LizardGPU_decompressFrame_device (those a batch hands on inside are [2]
 * of LizardGPU_framesDecodeDeviceStats), [3] stream-walk segments launched.  0 or -LIZARDGPU_ERR_*. */
int LizardGPU_streamDecodeDeviceStats(unsigned long long out[4]);

/* ---- SEEKABLE streams: a table of every item's place in a skippable frame at the END of the stream ----
 * Nothing in a stream says where frame k starts, so LizardGPU_decompressStream_device follows the chain with one wave, and a caller who
 * wants three items of a thousand decodes all of them.  A seekable stream ends in a SEEK TABLE (the idea of zstd's seekable format):
 * a skippable frame that every decoder of the format steps over — the reference's CLI folds the magic numbers 0x184D2A50 .. 5F into
 * "skippable" (programs/lizardio.c) — and from which a reader that knows it takes every item's place out of the stream's last bytes.
 * Opt-in on both sides: no entry above changes its bytes, its launches or its waits.
 *
 * The format, all fields little-endian; the table frame is the LAST thing in the stream:
 *     u32  0x184D2A5E (LIZARDGPU_SEEK_MAGIC)      skippable magic (tensor headers use ...54)
 *     u32  24 * n + 16                            bytes that follow
 *     n x  { u64 offset; u64 decodedBytes; u32 prefixBytes; u32 flags = 0 }        LizardGPU_seekEntry_t, 24 bytes
 *     u64  n     u32 version = 1     u32 0x4B535A4C ("LZSK", LIZARDGPU_SEEK_TAG)    the footer: the stream's last 16 bytes
 * Entry i describes ITEM i of the writing call: an opaque prefix of prefixBytes bytes (a tensor stream's tensor header; may be empty)
 * at `offset`, then one frame that decodes to decodedBytes bytes.  Item i ends where item i + 1 starts, the last item where the table
 * frame starts.  A table is USABLE for a stream of S bytes when the tag and the version match, the size field is 24 n + 16 and the
 * table frame is exactly the last 24 n + 24 bytes of the stream (tableOffset = S - (24 n + 24)), n >= 1, entry 0 starts at 0,
 * offset[i] + prefixBytes[i] < offset[i + 1] <= tableOffset (offset[n] standing for tableOffset), all flags are 0 and the sum of
 * decodedBytes does not wrap.  Anything else is "no usable table"; it is never an error of the stream, whose frames decode as before.
 * The CONCATENATION of two seekable streams is a valid stream whose table does not describe it, and these rules ALONE cannot say so:
 * the last table's offsets count from the second stream's start, and its last item "ends" where the table starts, so the rules
 * hold with a last item that swallows everything in between.  The decoder is what notices (below: the table locates, the decoder
 * validates): that item's frame does not fill its region, so LizardGPU_decompressSeekableStream_device falls back to the walk and
 * answers for the whole concatenation, and LizardGPU_decompressStreamItems_device refuses that item; the earlier indices name bytes
 * of the FIRST stream there.  Do not read items out of a concatenation; write one table over all items instead.
 * Out of scope: places INSIDE a frame (block-level tables).  Element ranges inside a tensor no longer are: Part 3d decodes them from
 * the blocks that cover them, walking the picked frame's record chain on the device.
 *
 * The host codec (lizard_seek_host.c; no device, no HIP):
 * LizardGPU_seekTableBytes(n): 24 n + 24, the bytes of the table frame for n items, or a code LizardGPU_frameIsError recognises
 * (GENERIC) when 24 n + 16 does not fit the u32 size field.
 * LizardGPU_seekTableWrite: the table frame for entries[0 .. n) into dst; the bytes written, or 0 (a null pointer, n == 0, no room in
 * dstCapacity, a size that does not fit).  It writes the entries as they are: whether a reader finds them usable is the caller's affair.
 * LizardGPU_seekTableRead judges the table from the LAST tailBytes bytes of a stream of streamBytes bytes (tail[0] is byte
 * streamBytes - tailBytes of the stream) and reads nothing outside tail[0 .. tailBytes):
 *   LIZARDGPU_SEEK_USABLE   *n items, the table frame starts at *tableOffset, the first min(*n, maxEntries) entries are in `entries`
 *                           (may be NULL with maxEntries 0): a caller whose array was too short sees *n > maxEntries and calls again.
 *   LIZARDGPU_SEEK_NONE     the stream does not end in the footer's tag (or is shorter than the shortest table frame, 48 bytes).
 *   LIZARDGPU_SEEK_MORE     the footer is there and its n plausible, but the tail is too short to judge the table: call again with
 *                           at least LizardGPU_seekTableBytes(*n) bytes of tail.  (A tail shorter than the 16-byte footer of a stream
 *                           of 48 bytes or more: *n = 0, i.e. "at least 24 bytes".)
 *   LIZARDGPU_SEEK_DAMAGED  the tag is there and a rule above fails.  The entries written so far are unspecified.
 * NONE and DAMAGED both mean "no usable table"; -LIZARDGPU_ERR_ARG for a null tail / n / tableOffset or tailBytes > streamBytes. */
typedef struct { uint64_t offset; uint64_t decodedBytes; uint32_t prefixBytes; uint32_t flags; } LizardGPU_seekEntry_t;
#define LIZARDGPU_SEEK_MAGIC   0x184D2A5Eu
#define LIZARDGPU_SEEK_TAG     0x4B535A4Cu
#define LIZARDGPU_SEEK_VERSION 1u
#define LIZARDGPU_SEEK_USABLE  0
#define LIZARDGPU_SEEK_NONE    1
#define LIZARDGPU_SEEK_MORE    2
#define LIZARDGPU_SEEK_DAMAGED 3
size_t LizardGPU_seekTableBytes(size_t n);
size_t LizardGPU_seekTableWrite(void* dst, size_t dstCapacity, const LizardGPU_seekEntry_t* entries, size_t n);
int    LizardGPU_seekTableRead(const void* tail, size_t tailBytes, uint64_t streamBytes, LizardGPU_seekEntry_t* entries, size_t maxEntries,
                               size_t* n, uint64_t* tableOffset);

/* The writer: LizardGPU_compressStream_device (Part 3) with the table behind it.  Same arguments, same refusals in the same order,
 * and d_dst[0 .. frameOffsets[nFrames]) is byte for byte that entry's stream for the same arguments; behind it the table frame of
 * LizardGPU_seekTableWrite over { frameOffsets[i], srcSizes[i], prefixSizes[i], 0 }.  The return value is the whole size,
 * frameOffsets[nFrames] (when asked for) where the TABLE starts, i.e. the plain entry's return value.
 * LizardGPU_compressStreamBound + LizardGPU_seekTableBytes(nFrames) bytes always suffice; dstMaxSize_tooSmall and "nothing outside
 * d_dst[0 .. dstCapacity) is written" hold as there.  Additionally GENERIC, before anything is launched, for a prefix of 2^32 bytes or
 * more or a table whose size field would not fit.  The host still waits ONCE: the table's bytes join the bytes the host knows, so
 * the device's one capacity test covers them, and one more kernel (lz_stream_seektable_kernel, one thread per entry) writes the table
 * behind the kernel that settles the frame offsets — nothing at all after an overflow.  Counted in LizardGPU_streamCompressDeviceStats. */
size_t LizardGPU_compressSeekableStream_device(void* d_dst, size_t dstCapacity, size_t nFrames, const void* const* d_srcs, const size_t* srcSizes,
                                               const void* const* prefixes, const size_t* prefixSizes, const LizardGPU_framePrefs_t* prefs,
                                               uint64_t* frameOffsets, size_t* failedFrame, void* stream);

/* The table of the stream at d_src (device memory): the footer comes down, then the table frame (two small copies, two waits, ordered
 * after what `stream` holds), and LizardGPU_seekTableRead judges it.  LIZARDGPU_SEEK_USABLE with *n, *tableOffset and the first
 * min(*n, maxEntries) entries as there, LIZARDGPU_SEEK_NONE or LIZARDGPU_SEEK_DAMAGED (never _MORE); a stream under 48 bytes is NONE
 * without a copy.  -LIZARDGPU_ERR_* for a null pointer or when the machinery fails. */
int LizardGPU_seekTable_device(const void* d_src, size_t srcSize, LizardGPU_seekEntry_t* entries, size_t maxEntries, size_t* n,
                               uint64_t* tableOffset, void* stream);

/* LizardGPU_decompressStream_device without the serial walk.  Signature and CONTRACT are that entry's: for every input — return value,
 * consumed bytes, frame count, decoded count, decoded bytes — the answer is what LizardGPU_decompressStream_device answers.
 * Fast path, when the table is usable and the sum of decodedBytes fits dstCapacity: ONE call of LizardGPU_decompressFrames_device over
 * all items, each item's frame with decodedBytes as its capacity at its packed place, each non-empty prefix as a frame of capacity
 * 0 (a skippable frame decodes to nothing).  It stands only if every frame answers EXACTLY its entry: result = decodedBytes (0 for a
 * prefix), consumed = its whole region.  The answer is then the sum, srcSize, and the batch's frames + 1 (the table frame).
 * On ANY deviation — no usable table, a sum above dstCapacity, one frame answering otherwise, a failure of the batch —
 * LizardGPU_decompressStream_device runs from the start and its answer is returned: the table locates, it never decides an answer. */
size_t LizardGPU_decompressSeekableStream_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, size_t* srcConsumedPtr,
                                                 size_t* nFramesPtr, size_t* decodedPtr, unsigned flags, void* stream);

/* Only the listed items of a seekable stream, decoded back to back into d_dst: items[0 .. nItems) are indices into the table,
 * STRICTLY ASCENDING; itemOffsets (may be NULL, else nItems + 1 host entries): where item items[k] starts in d_dst, and the total.
 * Returns the total or a code LizardGPU_frameIsError recognises.  The table locates, the decoder validates: every listed item's frame
 * (not its prefix, which is not read) goes through ONE LizardGPU_decompressFrames_device with decodedBytes as its capacity.
 *   - frameType_unknown: the stream has no usable table (nothing is decoded: use LizardGPU_decompressStream_device);
 *   - frameSize_wrong: items[k] >= the table's n; blockMode_invalid: items[k] <= items[k - 1]; *failedItem (may be NULL) = k for both,
 *     nothing is decoded;
 *   - dstMaxSize_tooSmall: the listed items' decodedBytes exceed dstCapacity, nothing is decoded;
 *   - an item whose frame does not answer exactly its entry: the frame's own error code, or decompressionFailed when it decoded to
 *     another size or did not fill its region; *failedItem = k of the first such item; what d_dst holds of other items is valid;
 *   - GENERIC for a null pointer or when the machinery fails.
 * nItems == 0 returns 0 and touches nothing.  Synchronous, ordered after what `stream` holds. */
size_t LizardGPU_decompressStreamItems_device(void* d_dst, size_t dstCapacity, const void* d_src, size_t srcSize, const size_t* items,
                                              size_t nItems, uint64_t* itemOffsets, size_t* failedItem, unsigned flags, void* stream);

/* Since process start, selected device: [0] LizardGPU_decompressSeekableStream_device calls answered through the table, [1] calls
 * that fell back to the walk, [2] items decoded by LizardGPU_decompressStreamItems_device, [3] tables read from device memory. */
int LizardGPU_seekDeviceStats(unsigned long long out[4]);

/* =====================================================================================================
 * Part 3c — tensor streams: element bytes split into planes before they are compressed.
 *
 * The bytes of a buffer of `size` bytes with element size E in {1, 2, 4, 8}, n = size / E elements, regrouped by significance
 * (what Blosc calls "shuffle"):  split writes dst[p * n + i] = src[i * E + p] for p < E, i < n and copies the size - n * E tail
 * bytes to dst + n * E; join is the exact inverse; E = 1 is a copy.  Interleaved, the exponent byte of a float is hidden from a
 * byte-oriented LZ parser and from huff0; in a plane of its own it has 2.7 bits of entropy for bf16 and fp32 weights.  With BYTE
 * planes fp16 gains nothing at these levels: its top byte holds 5.5 bits and the Huffman stage stores it raw (the bit planes
 * below are the filter for fp16).
 *
 * A batch of buffers in ONE launch each way (planes_kernels.h).  d_dsts, d_srcs, sizes, elemSizes: HOST arrays of nBuffers entries;
 * the pointers are device pointers on the selected device and may have any alignment (the kernels are fastest when both are
 * 16-byte aligned and n is a multiple of 16).  SYNCHRONOUS and ordered after what `stream` holds.  Nothing outside
 * d_dsts[i][0 .. sizes[i]) is written, nothing outside d_srcs[i][0 .. sizes[i]) is read.  NOT in place: a dst that overlaps a
 * src is the caller's error.  An entry of size 0 is allowed and skipped (its pointers may be NULL).
 * 0, or with NOTHING launched -LIZARDGPU_ERR_ARG: a null array, an elemSizes[i] outside {1, 2, 4, 8}, a null pointer in an entry
 * of non-zero size, a batch of 2^32 tiles (of 16 KiB) or more.  nBuffers == 0 returns 0 and touches nothing.  Strict like the rest:
 * no device or a HIP failure is -LIZARDGPU_ERR_* with LizardGPU_lastError set, never a host loop instead. */
int LizardGPU_splitPlanes_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs,
                                 const size_t* sizes, const uint32_t* elemSizes, void* stream);
int LizardGPU_joinPlanes_device (size_t nBuffers, void* const* d_dsts, const void* const* d_srcs,
                                 const size_t* sizes, const uint32_t* elemSizes, void* stream);
/* Since process start, selected device: [0] buffers split, [1] buffers joined, [2] bytes moved, [3] launches.  0 or -LIZARDGPU_ERR_*. */
int LizardGPU_planesStats(unsigned long long out[4]);

/* The tensor header: the format has no field that tells a reader which element size a frame's bytes were split with, so a tensor
 * stream puts a SKIPPABLE frame in front of every data frame.  Every decoder of the format steps over it (the reference's
 * LizardF_decompress, LizardGPU_decompressStream_device: a frame of 0 bytes that leaves the batch whole).  Its bytes:
 *     0 ..  3   LE32 magic LIZARDGPU_TENSOR_MAGIC (0x184D2A54, one of the format's sixteen skippable magics)
 *     4 ..  7   LE32 payload length = 40 + 8 * ndim
 *   payload:
 *     0 ..  3   "LZT1"
 *     4         elemSize: the element size the data frame's bytes were split with, 1 / 2 / 4 / 8 (1 = stored unsplit)
 *     5         ndim <= 8
 *     6 ..  7   zero
 *     8 .. 15   LE64 nbytes: the decoded size of the data frame that follows
 *    16 .. 39   the dtype's name, zero padded, at least one zero
 *    40 ..      ndim x LE64 dims
 * The data frame is an ordinary frame over the SPLIT bytes (LizardGPU_splitPlanes_device's layout for elemSize), so a reader
 * decodes it with any frame decoder and joins the planes.  Pure host code, no device.
 * Write: the header's bytes (48 + 8 * ndim), or 0 with nothing written: a null pointer, dstCapacity too small, elemSize not in
 * {1, 2, 4, 8}, ndim > 8, a dtype without a zero in its 24 bytes.
 * Read: 0 with *desc and *headerBytes filled (either may be NULL), or -LIZARDGPU_FRAME_ERR_frameType_unknown for anything that
 * is not such a header — a wrong magic, tag or length, ndim that disagrees with the length or exceeds 8, non-zero pad bytes, an
 * elemSize not in {1, 2, 4, 8}, a dtype name without a zero inside its field — or -LIZARDGPU_FRAME_ERR_frameHeader_incomplete
 * when srcSize ends inside the header (every field is judged as soon as the bytes in hand hold it, so a prefix of a valid header
 * is incomplete, never unknown). */
typedef struct { uint32_t elemSize; uint32_t ndim; uint64_t nbytes; uint64_t shape[8]; char dtype[24]; } LizardGPU_tensorDesc_t;
#define LIZARDGPU_TENSOR_MAGIC 0x184D2A54u
size_t LizardGPU_tensorHeaderWrite(void* dst, size_t dstCapacity, const LizardGPU_tensorDesc_t* desc); /* bytes, or 0 */
int    LizardGPU_tensorHeaderRead(const void* src, size_t srcSize, LizardGPU_tensorDesc_t* desc, size_t* headerBytes);

/* Bit planes: the second filter (what Blosc and HDF5 call "bitshuffle"), OPT-IN.  The BITS of a buffer regrouped by weight: with
 * n = size / E elements, n8 = n - n % 8 of them are transposed and a plane has P = n8 / 8 bytes.  Bit k (k < 8 E) of element i is
 * (src[i * E + k / 8] >> (k % 8)) & 1, the bit of weight 2^k of the little-endian element.
 *     split   dst[k * P + j] = sum over b < 8 of bit_k(element 8 j + b) << b     for k < 8 E, j < P
 *             the bytes src[n8 * E .. size) — the last n % 8 elements and the bytes behind the last whole element — are copied
 *             unchanged to dst[n8 * E .. size)
 *     join    the exact inverse
 * E = 1 is NOT a copy: it makes eight planes.  This is the bitshuffle library's bit order, applied to the whole buffer and not
 * block-wise, as the byte planes are.  A nearly constant bit plane is a long run, which the LZ parser alone removes, with no
 * Huffman stage, so the gain shows at level 10 already.  Stream / raw, reference library, 128 KiB blocks, randn(2^19) * 0.02
 * (profiles/bitplanes_ratio.json):
 *              level 10          level 21          level 30          level 41
 *              bytes   bits      bytes   bits      bytes   bits      bytes   bits
 *     fp16     1.0000  0.9375    1.0000  0.9375    1.0000  0.9375    1.0000  0.9375
 *     bf16     0.8431  0.7645    0.8244  0.7531    0.7456  0.7504    0.7252  0.7531
 *     fp32     0.9215  0.8825    0.9122  0.8766    0.8728  0.8753    0.8626  0.8766
 * Choose it for fp16 at any level and for weight-like bf16 / fp32 at levels 10 .. 29, which then reach level 30's ratio with
 * level 10's compressor and decoder.  It LOSES where the byte planes already feed huff0 well: bf16 randn * 1.0 (activation-like)
 * 0.8359 bytes / 0.8721 bits at level 10 and 0.7429 / 0.8081 at level 30; int32 indices below 50 000 are 0.5002 either way;
 * int64 arange(2^17) is 0.1107 bytes / 0.0043 bits at level 10.  A bf16 tensor of 8 KiB gains from neither at levels 10 and 30.
 * The default stays the byte planes.
 *
 * LizardGPU_splitBitPlanes_device / LizardGPU_joinBitPlanes_device: the signature and the whole contract of
 * LizardGPU_splitPlanes_device / LizardGPU_joinPlanes_device above (bitplanes_kernels.h; the host code is the same) — host arrays
 * of device pointers of any alignment, SYNCHRONOUS and ordered after what `stream` holds, entries of size 0 skipped, NOT in place,
 * nothing outside d_dsts[i][0 .. sizes[i]) written and nothing outside d_srcs[i][0 .. sizes[i]) read, -LIZARDGPU_ERR_ARG with
 * NOTHING launched for a null array, an elemSizes[i] outside {1, 2, 4, 8}, a null pointer in an entry of non-zero size or a batch
 * of 2^32 tiles or more, nBuffers == 0 returns 0.  LizardGPU_bitPlanesStats: their own counters — [0] buffers split, [1] buffers
 * joined, [2] bytes moved, [3] launches —, so LizardGPU_planesStats keeps counting byte-plane calls only. */
int LizardGPU_splitBitPlanes_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs,
                                    const size_t* sizes, const uint32_t* elemSizes, void* stream);
int LizardGPU_joinBitPlanes_device (size_t nBuffers, void* const* d_dsts, const void* const* d_srcs,
                                    const size_t* sizes, const uint32_t* elemSizes, void* stream);
int LizardGPU_bitPlanesStats(unsigned long long out[4]);

/* The tensor header with a filter.  LizardGPU_tensorHeaderWrite / Read above stay as they are, byte for byte, and go on refusing
 * the tag "LZT2": a v1 reader cannot undo a v2 filter.  LizardGPU_tensorDesc2_t: the v1 fields, then the filter; `reserved` is
 * written as zero and ignored on read.
 * Write2: filter LIZARDGPU_FILTER_BYTE_PLANES writes exactly LizardGPU_tensorHeaderWrite's "LZT1" bytes — streams made with byte
 * planes do not change and old readers read them; LIZARDGPU_FILTER_BIT_PLANES writes the same layout with the tag "LZT2", payload
 * byte 6 = 1 (the filter) and byte 7 = 0; any other filter writes nothing and returns 0, like every refusal of Write.
 * Read2: accepts "LZT1" (filter 0) and "LZT2" with payload byte 6 == 1 and byte 7 == 0; anything else under "LZT2" is
 * -LIZARDGPU_FRAME_ERR_frameType_unknown, so every meaning has ONE encoding.  Everything else as Read: every field is judged as soon
 * as the bytes in hand hold it, a prefix of a valid header is -LIZARDGPU_FRAME_ERR_frameHeader_incomplete, never unknown. */
#define LIZARDGPU_FILTER_BYTE_PLANES 0
#define LIZARDGPU_FILTER_BIT_PLANES  1
typedef struct { uint32_t elemSize; uint32_t ndim; uint64_t nbytes; uint64_t shape[8]; char dtype[24];
                 uint32_t filter; uint32_t reserved; } LizardGPU_tensorDesc2_t;
size_t LizardGPU_tensorHeaderWrite2(void* dst, size_t dstCapacity, const LizardGPU_tensorDesc2_t* desc); /* bytes, or 0 */
int    LizardGPU_tensorHeaderRead2(const void* src, size_t srcSize, LizardGPU_tensorDesc2_t* desc, size_t* headerBytes);

/* XOR with a base: the third filter, OPT-IN and per buffer, in front of either plane filter.  Callers rarely hold a tensor alone:
 * a checkpoint lies beside the previous one, a fine-tune beside its base model, a cache page beside its earlier version, and the
 * reader will hold that earlier version too.  XOR against it turns every unchanged bit into a zero, and the plane filters put those
 * zeros into runs.  For a buffer of `size` bytes with base b (`size` INTERLEAVED bytes, the earlier version as it lies in memory):
 *     split   dst = split(src XOR b)          join   dst = join(src) XOR b
 * where split / join are exactly the byte-plane or bit-plane layouts above; every byte takes part — whole elements, the ragged end
 * of the planes and the bytes behind the last whole element.  The XOR happens in registers (planes_kernels.h, bitplanes_kernels.h):
 * 3 bytes of memory traffic per payload byte where XOR-then-split through a temporary moves 5, and no third buffer.
 * Stream / raw, reference library, 128 KiB blocks, w = randn(2^19) * 0.02, the tensor w + step with |step| <= lr (an Adam-sized
 * update), the base w (profiles/xor_base_ratio.json; "bytes" / "bits" = the filter alone):
 *                                   level 10                            level 30
 *                                   bytes   XOR+bytes  bits    XOR+bits   bytes   XOR+bytes  bits    XOR+bits
 *     bf16, lr 1e-5 (14 % differ)   0.8430  0.3090     0.7638  0.3241     0.7455  0.1457     0.7501  0.1660
 *     fp16, lr 1e-5 (55 % differ)   1.0000  0.4935     0.9375  0.5074     1.0000  0.2793     0.9375  0.3323
 *     fp32, lr 1e-5 (all differ)    0.9215  0.6608     0.8818  0.6644     0.8728  0.5735     0.8751  0.5832
 *     bf16, lr 1e-4 (61 % differ)   0.8433  0.5180     0.7651  0.4783     0.7455  0.2897     0.7504  0.3477
 *     bf16, lr 1e-3 (96 % differ)   0.8431  0.6546     0.7632  0.6307     0.7454  0.5811     0.7500  0.5403
 *     bf16, 1 % replaced            0.8435  0.3753     0.7651  0.2122     0.7456  0.0751     0.7505  0.0890
 *     bf16, UNRELATED base          0.8431  0.9130     0.7645  0.7652     0.7456  0.7489     0.7504  0.7645
 * USE IT ONLY AGAINST A BASE THE DATA DERIVES FROM.  With an unrelated base it LOSES at level 10 with byte planes (0.9130 against
 * 0.8431) and roughly ties elsewhere; nothing chooses for the caller.  With a base, byte and bit planes are close; bytes are ahead
 * at level 30 for small updates.
 *
 * LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device: the whole contract of LizardGPU_splitPlanes_device /
 * LizardGPU_splitBitPlanes_device, `filter` (LIZARDGPU_FILTER_BYTE_PLANES / LIZARDGPU_FILTER_BIT_PLANES) choosing the layout — HOST
 * arrays of device pointers of any alignment (the bases too), ONE launch, SYNCHRONOUS and ordered after what `stream` holds, entries
 * of size 0 skipped (their pointers may be NULL), -LIZARDGPU_ERR_ARG with NOTHING launched for a null d_dsts / d_srcs / sizes /
 * elemSizes, an elemSizes[i] outside {1, 2, 4, 8}, a null src or dst in an entry of non-zero size, a batch of 2^32 tiles or more —
 * and for a `filter` that is neither value (judged first, for nBuffers == 0 as well); else nBuffers == 0 returns 0.
 * d_bases[i] == NULL: buffer i has no base; d_bases == NULL: none has; such a buffer's result is byte for byte the plain filter's,
 * in the same launch (a wave-uniform branch per tile).  Nothing outside d_bases[i][0 .. sizes[i]) is read.  A dst that overlaps a
 * src or a base is the caller's error; a base may be its buffer's src (the split is then all zeros).
 * LizardGPU_planesXorStats: these entries' own counters — [0] buffers split, [1] buffers joined, [2] payload bytes, [3] launches;
 * LizardGPU_planesStats / LizardGPU_bitPlanesStats keep counting the plain entries alone. */
int LizardGPU_splitPlanesXor_device(size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const void* const* d_bases,
                                    const size_t* sizes, const uint32_t* elemSizes, unsigned filter, void* stream);
int LizardGPU_joinPlanesXor_device (size_t nBuffers, void* const* d_dsts, const void* const* d_srcs, const void* const* d_bases,
                                    const size_t* sizes, const uint32_t* elemSizes, unsigned filter, void* stream);
int LizardGPU_planesXorStats(unsigned long long out[4]);

/* The tensor header of a tensor that was XORed with a base: tag "LZT3".  LizardGPU_tensorHeaderWrite / Read / Write2 / Read2 stay
 * byte for byte what they are and go on refusing "LZT3": a reader that cannot apply a base must not hand out the XORed bytes.
 * LizardGPU_tensorDesc3_t: the v2 fields with `reserved` named `flags`, then baseTag — an opaque number of the caller's (a step
 * number, a hash of their own) that the writer stores and a reader compares: it is how a reader learns that it was handed the wrong
 * base.  The library does not hash bases.  "LZT3" bytes: the "LZT2" layout with
 *   payload 6         the filter, 0 or 1
 *           7         the flags: LIZARDGPU_TENSOR_XOR_BASE (1)
 *          40 .. 47   LE64 baseTag
 *          48 ..      ndim x LE64 dims            payload length 48 + 8 * ndim
 * Write3: flags == 0 writes exactly Write2's bytes ("LZT1" / "LZT2") and refuses a non-zero baseTag; flags == 1 writes "LZT3"; any
 * other flags, and everything Write2 refuses, write nothing and return 0.  One encoding per meaning.
 * Read3: accepts all three tags; flags and baseTag come back as 0 for "LZT1" / "LZT2"; "LZT3" with byte 7 != 1 or byte 6 > 1 is
 * -LIZARDGPU_FRAME_ERR_frameType_unknown.  Every field is judged as soon as the bytes in hand hold it, so a prefix of a valid header
 * is -LIZARDGPU_FRAME_ERR_frameHeader_incomplete, never unknown: with fewer than 12 bytes a length is accepted when it is valid for
 * any of the three tags; once the tag is in hand the length and ndim must agree with that tag's fixed part (40 or 48). */
#define LIZARDGPU_TENSOR_XOR_BASE 1u
typedef struct { uint32_t elemSize; uint32_t ndim; uint64_t nbytes; uint64_t shape[8]; char dtype[24];
                 uint32_t filter; uint32_t flags; uint64_t baseTag; } LizardGPU_tensorDesc3_t;
size_t LizardGPU_tensorHeaderWrite3(void* dst, size_t dstCapacity, const LizardGPU_tensorDesc3_t* desc); /* bytes, or 0 */
int    LizardGPU_tensorHeaderRead3(const void* src, size_t srcSize, LizardGPU_tensorDesc3_t* desc, size_t* headerBytes);

/* ============================================================================================================================
 * Part 3d — a row range of a tensor, decoded from the blocks that cover it.
 * ============================================================================================================================
 * A sharded loader wants rows [start, stop) of every weight.  Every frame this library writes has independent blocks and every
 * record but the last decodes to exactly the frame's block size B, so byte x of the decoded content lies in record x / B: a reader
 * decodes the records that cover the bytes it needs and joins that element range only.  Three entries, each usable alone.  Block-level
 * tables stay out of scope: the record chain of a picked frame is walked on the device, as the batch decoder walks it.
 *
 * 1. The arithmetic (lizard_slice_host.c; no device, no HIP).
 * LizardGPU_planesRangeBytes: the byte ranges [lo, hi) of the SPLIT content that elements [first, last) of a buffer of nElems elements
 * of elemSize bytes (1, 2, 4 or 8) need, ascending, in PIECE ORDER:
 *   LIZARDGPU_FILTER_BYTE_PLANES   elemSize ranges, one per plane: [p * nElems + first, p * nElems + last).  An element size of 1 —
 *                                  also a tensor stored unsplit — is one range.
 *   LIZARDGPU_FILTER_BIT_PLANES    8 * elemSize + 1 ranges.  With n8 = nElems - nElems % 8 and P = n8 / 8, one per plane:
 *                                  [k * P + first / 8, k * P + ceil(min(last, n8) / 8)), empty (lo == hi) when first >= min(last, n8);
 *                                  then one over the raw elements behind n8 * elemSize that belong to the range:
 *                                  [max(first, n8) * elemSize, last * elemSize) when last > n8, else empty.
 * Every range holds exactly the bytes in which some element of the range has a bit.  Returns the number of ranges; 0 for a null
 * `out`, another element size or filter, first > last, last > nElems, or maxOut below that number.
 * LizardGPU_frameRangesBound: the room the covering blocks of `ranges` take in a frame of block size blockSize: the sum over the
 * ranges of (ceil(hi / B) - floor(lo / B)) * B, nothing for an empty range.  0 for a null pointer or a block size of 0.
 *
 * 2. LizardGPU_decompressFrameRanges_device: of nFrames frames in device memory, decode only the records that cover the byte ranges
 * ranges[frames[f].firstRange .. + frames[f].nRanges) of frame f's decoded content, into ONE device buffer.  Let full_f be what
 * LizardGPU_decompressFrame_device decodes for frame f with room enough.  For every frame with results[f] == 0 and every one of its
 * ranges r = [lo, hi):   d_dst[rangeAt[r] + lo % B + i] == full_f[lo + i] for i < hi - lo,
 * B being the frame's block size.  The whole covering blocks of range r lie back to back from rangeAt[r], every one in a slot of B
 * bytes (the last block of a frame fills less of its slot); ranges are placed in index order, rangeAt[nRanges] is the total —
 * nRanges here being the largest firstRange + nRanges of the call, which `ranges` and `rangeAt` (one entry more) must hold.  An empty
 * range takes no room and decodes nothing.  A block that two ranges of a frame both touch is decoded once per range: at most one
 * extra block per range.  Nothing outside d_dst[0 .. dstCapacity) is written, nothing outside a frame's d_src[0 .. srcSize) is read.
 * In this order: the frames are walked side by side, one wave each (the count pass of LizardGPU_decompressFrames_device); the host
 * turns the ranges into a list of picked records; the same walk fills the record tables and ONE launch decodes the picks, one wave
 * each.  The host waits twice per call, whatever the number of frames and ranges.
 * The total is known after the count pass and is tested against dstCapacity before anything that writes d_dst is launched: a total
 * above it returns -LIZARDGPU_ERR_ARG with "dstMaxSize_tooSmall" in LizardGPU_lastError and d_dst untouched; a frame refused before
 * keeps its code, every other answers GENERIC.
 * The ranges of a frame refused in the count pass take no room.
 * Per frame, results[f] is 0 or a code LizardGPU_frameIsError recognises; a refused frame does not stop the others and its bytes in
 * d_dst are unspecified:
 *   the walk's own code        for a chain it refuses (a cut frame, a bad header ...)
 *   frameType_unknown          a skippable frame
 *   frameSize_wrong            a header without content size C on a frame that has records (a frame without records has C = 0); a
 *                              record count other than ceil(C / B); a range with lo > hi or hi > C
 *   decompressionFailed        a picked record fails, needs its history (a linked frame), or decodes to anything but B bytes — for the
 *                              frame's last record, C - (n - 1) * B bytes
 *   GENERIC                    a null d_src with a non-zero srcSize
 * A range belongs to at most one frame (else -LIZARDGPU_ERR_ARG); a range of no frame takes no room.
 * The return value is 0 when the call did its work (LizardGPU_lastError names the first refused frame), -LIZARDGPU_ERR_*
 * otherwise, and then every results[f] is an error code.
 * LIMITS, which follow from decoding a part: (1) the content checksum of a frame is NEVER verified here — a slice cannot verify
 * it; (2) damage in a record that is not picked is not seen; (3) a foreign frame may hold a short record in the middle among the
 * records that were not picked and still have the right record count — a flushed frame — which cannot be told from a frame of full
 * blocks without decoding everything: the entry is for frames in which every record but the last fills the block, which is every
 * frame this library writes.
 * LizardGPU_sliceDeviceStats: [0] records decoded, [1] frames answered, [2] frames refused, [3] calls; since process start.
 *
 * 3. LizardGPU_joinPlanesRange_device: for every item, d_dst[0 .. (last - first) * elemSize) receives
 * join(the split bytes)[first * elemSize .. last * elemSize) — the join of LizardGPU_joinPlanes_device or
 * LizardGPU_joinBitPlanes_device, by `filter` — read from PIECES: d_pieces is a HOST array of device addresses, and
 * d_pieces[firstPiece + q] is the address of the FIRST BYTE of range q of LizardGPU_planesRangeBytes for that item (its `lo`), at any
 * byte address: a piece starts anywhere inside a decoded block.  An empty range's piece is never read and may be NULL.  With d_base
 * not NULL the result is XORed with d_base[0 .. (last - first) * elemSize): the caller passes the base already advanced to element
 * `first`.  ONE launch serves the batch, in the manner of Part 3c: tiles numbered through the batch, a wave per tile, the item found
 * by bisection.  Nothing outside an item's d_dst bytes is written; nothing is read but the bytes of its ranges and of its base.
 * Empty items (first == last) are skipped.  -LIZARDGPU_ERR_ARG with nothing launched for a null array, an element size outside
 * {1, 2, 4, 8}, a filter that is neither, first > last or last > nElems, a null d_dst or a null piece of a non-empty range, or a
 * batch of 2^32 tiles or more.  `reserved` must be 0.  Column ranges and other strided slices are out of scope. */
typedef struct { uint64_t lo, hi; } LizardGPU_byteRange_t;
size_t LizardGPU_planesRangeBytes(uint64_t nElems, uint32_t elemSize, uint32_t filter, uint64_t first, uint64_t last,
                                  LizardGPU_byteRange_t* out, size_t maxOut);
size_t LizardGPU_frameRangesBound(const LizardGPU_byteRange_t* ranges, size_t nRanges, size_t blockSize);
typedef struct { const void* d_src; size_t srcSize; uint32_t firstRange, nRanges; } LizardGPU_sliceFrame_t;
int LizardGPU_decompressFrameRanges_device(void* d_dst, size_t dstCapacity, size_t nFrames, const LizardGPU_sliceFrame_t* frames,
                                           const LizardGPU_byteRange_t* ranges, uint64_t* rangeAt /* nRanges + 1, host, out */,
                                           size_t* results /* nFrames, host: 0 or a frame error code */, void* stream);
int LizardGPU_sliceDeviceStats(unsigned long long out[4]);
typedef struct { void* d_dst; const void* d_base; uint64_t nElems, first, last; uint32_t elemSize, filter, firstPiece, reserved; } LizardGPU_planesRange_t;
int LizardGPU_joinPlanesRange_device(size_t nItems, const LizardGPU_planesRange_t* items, const void* const* d_pieces, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIZARD_AMD_H */
