// tests/pack_kernels.hip — TEST INFRASTRUCTURE: lz_scan_kernel and lz_gather_kernel (lizard_amd/csrc/lz_pack.h) on their own, against a
// sequential host model, on synthetic size arrays.  The pipelines reach these kernels only with the sizes real compressors produce;
// here the sizes sit on the kernels' edges: more than 1024 blocks (the scan's per-thread stretch, threads whose range clamps to
// nBlocks), a total above 2^32, lengths around the 16-byte lane copy and the 4096-byte pass of the gather, odd slot strides (unaligned
// sources, destinations on every residue mod 16), and the frame mode's stored-raw rule at cs = 0, n - 2, n - 1, n, n + 5 and n = 1.
// The model is the one of tests/pipeline_fake.c, restated.  Offsets are compared entry by entry, the packed buffer byte by byte, with
// 64-byte canaries on both sides of each.  Every HIP call is checked; the program stops at the first error.
//   hipcc -O2 --offload-arch=gfx950 tests/pack_kernels.hip -o tests/pack_kernels        prints "cases: N mismatches: 0", exit 0
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lizard_amd/csrc/lz_pack.h"

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "pack_kernels: %s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

namespace {
const size_t kGuard = 64;
const uint8_t kCanary = 0xC3;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
int g_cases, g_bad;

void mismatch(const char* what, uint32_t nb, int mode, uint64_t at, uint64_t got, uint64_t want)
{
    if (g_bad++ < 20) fprintf(stderr, "pack_kernels: %s: nBlocks %u mode %d: at %llu got %llu, want %llu\n", what, nb, mode,
                              (unsigned long long)at, (unsigned long long)got, (unsigned long long)want);
}

// a device buffer of n bytes between two canaries
struct Dev {
    uint8_t* base = nullptr; size_t n = 0;
    explicit Dev(size_t bytes) : n(bytes) { CK(hipMalloc((void**)&base, n + 2 * kGuard)); CK(hipMemset(base, kCanary, n + 2 * kGuard)); }
    ~Dev() { CK(hipFree(base)); }
    uint8_t* p() const { return base + kGuard; }
    void put(const void* h) { if (n) CK(hipMemcpy(p(), h, n, hipMemcpyHostToDevice)); }
    std::vector<uint8_t> get(const char* what, uint32_t nb, int mode) const
    {
        std::vector<uint8_t> h(n + 2 * kGuard);
        CK(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kGuard; i++) {
            if (h[i] != kCanary) mismatch(what, nb, mode, i, h[i], kCanary);
            if (h[kGuard + n + i] != kCanary) mismatch(what, nb, mode, kGuard + n + i, h[kGuard + n + i], kCanary);
        }
        return std::vector<uint8_t>(h.begin() + kGuard, h.begin() + kGuard + n);
    }
};

// the rule of the frame layer, restated: a block is stored raw when it did not shrink below its input; a 1-byte block never is
bool model_raw(uint32_t n, uint32_t cs) { return n != 1u && (cs == 0u || cs >= n); }
uint64_t model_record(uint32_t n, uint32_t cs, int mode) { return mode == LZ_PACK_PAYLOAD ? cs : 4ull + (model_raw(n, cs) ? n : cs); }
std::vector<uint64_t> model_offsets(const std::vector<uint32_t>& sizes, uint32_t blockSize, uint32_t last, int mode)
{
    std::vector<uint64_t> o(sizes.size() + 1);
    uint64_t run = 0;
    for (size_t b = 0; b < sizes.size(); b++) { o[b] = run; run += model_record(b + 1 == sizes.size() ? last : blockSize, sizes[b], mode); }
    o[sizes.size()] = run;
    return o;
}

void compare_offsets(const Dev& d_offsets, const std::vector<uint64_t>& want, uint32_t nb, int mode)
{
    const std::vector<uint8_t> raw = d_offsets.get("offsets canary", nb, mode);
    for (size_t i = 0; i <= nb; i++) {
        uint64_t got;
        memcpy(&got, raw.data() + 8 * i, 8);
        if (got != want[i]) mismatch("offsets", nb, mode, i, got, want[i]);
    }
}

// lz_scan_kernel alone
void scan_case(const std::vector<uint32_t>& sizes, uint32_t blockSize, uint32_t last, int mode)
{
    const uint32_t nb = (uint32_t)sizes.size();
    Dev d_sizes(4 * (size_t)nb), d_offsets(8 * ((size_t)nb + 1));
    d_sizes.put(sizes.data());
    hipLaunchKernelGGL(lz_scan_kernel, dim3(1), dim3(1024), 0, 0, (const u32*)d_sizes.p(), (u64*)d_offsets.p(), nb, blockSize, last, mode);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    compare_offsets(d_offsets, model_offsets(sizes, blockSize, last, mode), nb, mode);
    g_cases++;
}

// lz_pack_launch: scan + gather.  Every non-raw size is at most `stride`, so the gather reads inside its slot; the input has
// (nb - 1) * blockSize + last bytes, all a raw record reads.
void pack_case(const std::vector<uint32_t>& sizes, size_t stride, uint32_t blockSize, uint32_t last, int mode)
{
    const uint32_t nb = (uint32_t)sizes.size();
    const size_t inBytes = mode == LZ_PACK_FRAME ? (size_t)(nb - 1) * blockSize + last : 0;
    std::vector<uint8_t> slots((size_t)nb * stride), in(inBytes);
    for (auto& v : slots) v = (uint8_t)(rnd() | 1u);             // (odd bytes in the slots, even ones in the input: the source shows in every byte)
    for (auto& v : in) v = (uint8_t)(rnd() & ~1u);
    const std::vector<uint64_t> want = model_offsets(sizes, blockSize, last, mode);
    std::vector<uint8_t> packed((size_t)want[nb]);
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t n = b + 1 == nb ? last : blockSize, cs = sizes[b];
        uint8_t* out = packed.data() + want[b];
        const uint8_t* from = slots.data() + (size_t)b * stride;
        uint32_t len = cs;
        if (mode == LZ_PACK_FRAME) {
            const bool raw = model_raw(n, cs);
            const uint32_t word = raw ? (n | 0x80000000u) : cs;
            if (n == 1u && (word >> 31)) { fprintf(stderr, "pack_kernels: the model stores a 1-byte block raw\n"); exit(2); }
            out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
            out += 4;
            if (raw) { from = in.data() + (size_t)b * blockSize; len = n; }
        }
        if (!(mode == LZ_PACK_FRAME && model_raw(n, cs)) && len > stride) { fprintf(stderr, "pack_kernels: a case reads outside its slot\n"); exit(2); }
        if (len) memcpy(out, from, len);
    }
    Dev d_sizes(4 * (size_t)nb), d_offsets(8 * ((size_t)nb + 1)), d_slots(slots.size()), d_in(in.size()), d_packed(packed.size());
    d_sizes.put(sizes.data()); d_slots.put(slots.data()); d_in.put(in.data());
    lz_pack_launch(d_in.p(), d_slots.p(), stride, (const u32*)d_sizes.p(), (u64*)d_offsets.p(), d_packed.p(), nb, blockSize, last, mode, 0);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    compare_offsets(d_offsets, want, nb, mode);
    const std::vector<uint8_t> got = d_packed.get("packed canary", nb, mode);
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != packed[i]) { mismatch("packed bytes", nb, mode, i, got[i], packed[i]); break; }
    if (d_slots.get("slots canary", nb, mode) != slots) mismatch("the slots changed", nb, mode, 0, 0, 0);
    g_cases++;
}
}  // namespace

int main()
{
    int dev = 0;
    CK(hipGetDevice(&dev));
    // ---- the scan alone: the per-thread stretch per = ceil(nBlocks / 1024) matters above 1024 blocks ----
    static const uint32_t scanBlocks[] = { 1, 2, 63, 1023, 1024, 1025, 2047, 2048, 2049, 5000, 70001 };
    for (uint32_t nb : scanBlocks)
        for (int mode = 0; mode < 2; mode++)
            for (int rep = 0; rep < 2; rep++) {
                const uint32_t blockSize = 4099, last = rep ? 1u + rnd() % blockSize : blockSize;
                std::vector<uint32_t> sizes(nb);
                for (auto& v : sizes) { const uint32_t r = rnd(); v = (r & 7u) == 0 ? 0u : (r & 7u) == 1 ? blockSize - 1u + (r >> 8) % 3u : (r >> 8) % (blockSize + 6u); }
                scan_case(sizes, blockSize, last, mode);
            }
    {   // a total above 2^32: the running sums are 64-bit
        const std::vector<uint32_t> huge(5, 0x7FFFFFFFu);
        scan_case(huge, 0x7FFFFFFFu, 0x7FFFFFFFu, LZ_PACK_PAYLOAD);
        std::vector<uint32_t> many(3000, 0x00200000u);
        scan_case(many, 0x00200000u, 0x00200000u, LZ_PACK_PAYLOAD);
    }
    // ---- scan + gather, payload mode: odd strides, lengths around the 16-byte copy and the 4096-byte pass ----
    static const size_t strides[] = { 272, 8209 };
    static const uint32_t edge[] = { 0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097 };
    static const uint32_t packBlocks[] = { 1, 7, 1025, 2049 };
    for (size_t stride : strides)
        for (uint32_t nb : packBlocks)
            for (int rep = 0; rep < (nb > 1000 ? 3 : 12); rep++) {
                std::vector<uint32_t> sizes(nb);
                for (auto& v : sizes) {
                    const uint32_t r = rnd(), pick = (r >> 4) % 14u;
                    v = pick < 11u ? edge[pick] : pick == 11u ? (uint32_t)stride : (r >> 8) % ((uint32_t)stride + 1u);
                    if (v > stride) v = (uint32_t)stride - (r >> 8) % 40u;
                }
                if (nb == 1) sizes[0] = rep < 11 ? edge[rep] > stride ? (uint32_t)stride : edge[rep] : (uint32_t)stride;
                pack_case(sizes, stride, 0, 0, LZ_PACK_PAYLOAD);
            }
    // ---- scan + gather, frame mode: the record word, the raw bit and the source at the edges of the stored-raw rule ----
    static const uint32_t lasts[] = { 1, 2, 4099 };
    const uint32_t blockSize = 4099;
    const size_t frameStride = 4111;                            // odd, and at least n - 1: a block that shrank by one byte fits its slot
    for (uint32_t last : lasts)
        for (uint32_t nb : packBlocks)
            for (int rep = 0; rep < (nb > 1000 ? 2 : 6); rep++) {
                std::vector<uint32_t> sizes(nb);
                for (uint32_t b = 0; b < nb; b++) {
                    const uint32_t n = b + 1 == nb ? last : blockSize;
                    const uint32_t pick = nb <= 7 ? (b + (uint32_t)rep) % 6u : rnd() % 6u;
                    const uint32_t choice[6] = { 0u, 1u, n >= 2u ? n - 2u : 0u, n - 1u, n, n + 5u };
                    sizes[b] = choice[pick];
                }
                pack_case(sizes, frameStride, blockSize, last, LZ_PACK_FRAME);
            }
    printf("cases: %d mismatches: %d\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
