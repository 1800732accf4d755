// tests/unframes_kernels.hip — TEST INFRASTRUCTURE: lz_unframes_settle_kernel and lz_unframes_finish_kernel
// (lizard_amd/csrc/unframes_kernels.h) on their own, against a sequential host model, on synthetic tables, followed by
// lz_xxh32_frames_kernel (lz_frames_pack.h) between them as in LizardGPU_decompressFrames_device.  That entry reaches these kernels only
// with the results real frames produce.  Here: batches of 1, 3, 4, 5, 255, 256, 257 and 1030 frames whose record counts are 0, 1, 2, 63,
// 64, 65, 128, 129 and 130; per-record results that are all full, short in the last record only, short in the middle, failed
// (0xFFFFFFFF) or in need of history (0xFFFFFFFE) at the first, a middle or the last record; entries that are not to be decoded between
// the others; content sizes that match, differ or are absent; stored checksums that match or differ at frame ends of every address
// residue, with and without the verify flag.  "Decoded" bytes are random, so the hash over them is compared with Lizard_XXH32 of
// lizard_amd/csrc/lizard_xxhash.c compiled into the program.  64-byte canaries surround every table.  Every HIP call is checked.
//   hipcc -O2 --offload-arch=gfx950 tests/unframes_kernels.hip lizard_amd/csrc/lizard_xxhash.c -o tests/unframes_kernels
//   prints "cases: N mismatches: 0", exit 0
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lizard_amd/csrc/lz_frames_pack.h"
#include "../lizard_amd/csrc/unframes_kernels.h"

extern "C" unsigned int Lizard_XXH32(const void* input, size_t length, unsigned int seed);

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "unframes_kernels: %s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

namespace {
const size_t kGuard = 64;
const uint8_t kCanary = 0xC3;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
int g_cases, g_bad;

void mismatch(const char* what, size_t at, uint64_t got, uint64_t want)
{
    if (g_bad++ < 20) fprintf(stderr, "unframes_kernels: %s: at %zu got %llu, want %llu\n", what, at, (unsigned long long)got, (unsigned long long)want);
}

struct Dev {
    uint8_t* base = nullptr; size_t n = 0;
    explicit Dev(size_t bytes) : n(bytes) { CK(hipMalloc((void**)&base, n + 2 * kGuard)); CK(hipMemset(base, kCanary, n + 2 * kGuard)); }
    Dev(const Dev&) = delete;
    ~Dev() { CK(hipFree(base)); }
    uint8_t* p() const { return base + kGuard; }
    void put(const void* h) { if (n) CK(hipMemcpy(p(), h, n, hipMemcpyHostToDevice)); }
    std::vector<uint8_t> get(const char* what) const
    {
        std::vector<uint8_t> h(n + 2 * kGuard);
        CK(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kGuard; i++) {
            if (h[i] != kCanary) mismatch(what, i, h[i], kCanary);
            if (h[kGuard + n + i] != kCanary) mismatch(what, kGuard + n + i, h[kGuard + n + i], kCanary);
        }
        return std::vector<uint8_t>(h.begin() + kGuard, h.begin() + kGuard + n);
    }
};

const uint32_t kCounts[] = { 0, 1, 2, 63, 64, 65, 128, 129, 130 };
const uint32_t kBlock = 48;                                  // the "block size" of the synthetic frames: sizes stay small

void run(uint32_t F)
{
    std::vector<LzUnframesEntry> frames(F);
    std::vector<LzFramesEntry> hash(F);
    std::vector<uint32_t> out;
    std::vector<uint8_t> dst, src;
    std::vector<LzUnframesResult> wantSettle(F), want(F);
    std::vector<uint64_t> wantHashBytes(F);
    memset(frames.data(), 0, F * sizeof frames[0]);
    memset(hash.data(), 0, F * sizeof hash[0]);
    // the shapes first, then the buffers (addresses are known only once they are allocated)
    std::vector<size_t> dstAt(F), srcAt(F);
    for (uint32_t f = 0; f < F; f++) {
        LzUnframesEntry& e = frames[f];
        const uint32_t n = kCounts[(f + F) % 9], kind = rnd() % 8;
        e.first = out.size(); e.nRecords = n; e.maxBlock = kBlock;
        e.flags = rnd() % 7 == 0 ? LZU_WALK : LZU_DECODE | (rnd() % 3 ? LZU_VERIFY : 0u);
        for (uint32_t i = 0; i < n; i++) out.push_back(kBlock);
        if (n) {
            uint32_t* o = out.data() + e.first;
            const uint32_t where = kind & 1 ? n - 1 : kind & 2 ? 0 : n / 2;
            if (kind == 1) o[n - 1] = rnd() % kBlock;                        // short last: clean
            else if (kind == 2) o[where] = 0xFFFFFFFFu;
            else if (kind == 3) o[where] = 0xFFFFFFFEu;
            else if (kind == 4 && n > 1) o[rnd() % (n - 1)] = kBlock - 1;    // short in the middle
            else if (kind == 5) o[where] = rnd() & 1 ? 0xFFFFFFFFu : 0xFFFFFFFEu;
            else if (kind >= 6) o[n / 2] = kind == 6 ? 0xFFFFFFFFu : 0xFFFFFFFEu;
        }
        bool clean = true;
        uint64_t size = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t v = out[e.first + i];
            if (v >= 0xFFFFFFFEu || (i + 1 < n && v != kBlock)) clean = false;
            else size += v;
        }
        wantSettle[f].size = 0; wantSettle[f].state = LZU_DEAD; wantSettle[f].reserved = 0;
        if (e.flags & LZU_DECODE) { wantSettle[f].state = clean ? LZU_CLEAN : LZU_DELEGATE; wantSettle[f].size = clean ? size : 0; }
        wantHashBytes[f] = wantSettle[f].size;
        const uint32_t cs = rnd() % 4;
        e.contentSize = cs == 0 ? 0 : cs == 1 && clean ? size + 1 : clean ? size : 5;
        e.cap = (uint64_t)n * kBlock;
        dstAt[f] = dst.size() + (f % 5);
        dst.resize(dstAt[f] + e.cap + 3);
        e.frameBytes = 11 + rnd() % 40;
        e.srcSize = e.frameBytes + rnd() % 3;
        srcAt[f] = src.size() + (f % 3);
        src.resize(srcAt[f] + e.srcSize + 1);
    }
    for (auto& b : dst) b = (uint8_t)rnd();
    for (auto& b : src) b = (uint8_t)rnd();
    Dev dDst(dst.size()), dSrc(src.size());
    for (uint32_t f = 0; f < F; f++) {
        LzUnframesEntry& e = frames[f];
        e.dst = (uint64_t)(uintptr_t)(dDst.p() + dstAt[f]); e.src = (uint64_t)(uintptr_t)(dSrc.p() + srcAt[f]);
        hash[f].src = e.dst; hash[f].srcSize = 0xDEADull;
        if (e.flags & LZU_VERIFY) hash[f].flags = LZK_FRAMES_LIVE | LZK_FRAMES_CHECKSUM;
        want[f] = wantSettle[f];
        if (want[f].state == LZU_CLEAN) {
            const uint32_t h = Lizard_XXH32(dst.data() + dstAt[f], (size_t)want[f].size, 0);
            const bool wrongSum = rnd() % 3 == 0;
            const uint32_t stored = wrongSum ? h ^ (1u << (rnd() % 32)) : h;
            uint8_t* s = src.data() + srcAt[f] + e.frameBytes - 4;
            s[0] = (uint8_t)stored; s[1] = (uint8_t)(stored >> 8); s[2] = (uint8_t)(stored >> 16); s[3] = (uint8_t)(stored >> 24);
            if (e.contentSize && e.contentSize != want[f].size) want[f].state = LZU_DELEGATE;
            else if ((e.flags & LZU_VERIFY) && wrongSum) want[f].state = LZU_DELEGATE;
            if (want[f].state != LZU_CLEAN) want[f].size = 0;
        }
    }
    dDst.put(dst.data()); dSrc.put(src.data());
    Dev dFrames(F * sizeof frames[0]), dHash(F * sizeof hash[0]), dOut(out.size() * 4), dRes(F * sizeof(LzUnframesResult));
    dFrames.put(frames.data()); dHash.put(hash.data()); dOut.put(out.data());
    const LzUnframesEntry* df = (const LzUnframesEntry*)dFrames.p();
    LzFramesEntry* dh = (LzFramesEntry*)dHash.p();
    LzUnframesResult* dr = (LzUnframesResult*)dRes.p();
    hipLaunchKernelGGL(lz_unframes_settle_kernel, dim3((F + LZU_WALK_WAVES - 1) / LZU_WALK_WAVES), dim3(64 * LZU_WALK_WAVES), 0, 0, df, F, (const u32*)dOut.p(), dr, dh);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    {
        std::vector<uint8_t> r = dRes.get("settle: result records"), h = dHash.get("settle: hash table");
        const LzUnframesResult* got = (const LzUnframesResult*)r.data();
        const LzFramesEntry* gh = (const LzFramesEntry*)h.data();
        for (uint32_t f = 0; f < F; f++) {
            if (got[f].state != wantSettle[f].state) mismatch("settle: state", f, got[f].state, wantSettle[f].state);
            if (got[f].size != wantSettle[f].size) mismatch("settle: size", f, got[f].size, wantSettle[f].size);
            if (gh[f].srcSize != wantHashBytes[f]) mismatch("settle: bytes to hash", f, gh[f].srcSize, wantHashBytes[f]);
            LzFramesEntry a = gh[f], b = hash[f];
            a.srcSize = b.srcSize = 0;
            if (memcmp(&a, &b, sizeof a)) mismatch("settle: the rest of a hash entry changed", f, 1, 0);
        }
    }
    lz_frames_hash_launch(dh, F, 0);
    CK(hipGetLastError());
    hipLaunchKernelGGL(lz_unframes_finish_kernel, dim3((F + 255) / 256), dim3(256), 0, 0, df, F, (const LzFramesEntry*)dh, dr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    {
        std::vector<uint8_t> r = dRes.get("finish: result records");
        const LzUnframesResult* got = (const LzUnframesResult*)r.data();
        for (uint32_t f = 0; f < F; f++) {
            if (got[f].state != want[f].state) mismatch("finish: state", f, got[f].state, want[f].state);
            if (got[f].size != want[f].size) mismatch("finish: size", f, got[f].size, want[f].size);
        }
        if (dFrames.get("frame table") != std::vector<uint8_t>((uint8_t*)frames.data(), (uint8_t*)(frames.data() + F))) mismatch("the frame table changed", 0, 1, 0);
        if (dOut.get("per-record results") != std::vector<uint8_t>((uint8_t*)out.data(), (uint8_t*)(out.data() + out.size()))) mismatch("the per-record results changed", 0, 1, 0);
        if (dDst.get("decoded bytes") != dst) mismatch("the decoded bytes changed", 0, 1, 0);
        if (dSrc.get("frames") != src) mismatch("the frames changed", 0, 1, 0);
    }
    g_cases += (int)F;
}
}  // namespace

int main()
{
    const uint32_t batches[] = { 1, 3, 4, 5, 255, 256, 257, 1030 };
    for (int round = 0; round < 3; round++)
        for (uint32_t F : batches) run(F);
    printf("cases: %d mismatches: %d\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
