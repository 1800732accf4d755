// tests/frame_pack_kernels.hip — TEST INFRASTRUCTURE: lz_frame_scan_kernel and lz_frame_gather_kernel (lizard_amd/csrc/lz_frame_pack.h)
// on their own, against a sequential host model, on synthetic size arrays.  LizardGPU_compressFrame_device reaches these kernels only
// with the sizes real compressors produce and with capacities its bound allows; here the cursor is carried over three successive
// launches from starts on every residue mod 16, the scan starts above 2^32 (offsets only: no buffer is that large), a chunk has more
// than 1024 blocks, the stored-raw rule sits on its edges (cs = 0, 1, n - 2, n - 1, n, n + 5; n = 1), and the byte limit falls exactly
// on a record's end, one byte before it, and inside the first record: the flag must rise, nothing at or behind the limit may change,
// the records in front of it must be whole.  The destination is allocated for the WHOLE frame whatever the limit, so a kernel that
// ignored the limit would be caught by a comparison, not by a fault.  64-byte canaries surround every buffer.  Every HIP call is
// checked; the program stops at the first error.
//   hipcc -O2 --offload-arch=gfx950 tests/frame_pack_kernels.hip -o tests/frame_pack_kernels     prints "cases: N mismatches: 0", exit 0
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lizard_amd/csrc/lz_frame_pack.h"

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "frame_pack_kernels: %s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

namespace {
const size_t kGuard = 64;
const uint8_t kCanary = 0xC3;
const uint64_t kNoLimit = ~0ull;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
int g_cases, g_bad;

void mismatch(const char* what, const char* name, uint64_t at, uint64_t got, uint64_t want)
{
    if (g_bad++ < 20) fprintf(stderr, "frame_pack_kernels: %s: %s: at %llu got %llu, want %llu\n", name, what,
                              (unsigned long long)at, (unsigned long long)got, (unsigned long long)want);
}

// a device buffer of n bytes between two canaries
struct Dev {
    uint8_t* base = nullptr; size_t n = 0;
    explicit Dev(size_t bytes, uint8_t fill = kCanary) : n(bytes)
    {
        CK(hipMalloc((void**)&base, n + 2 * kGuard));
        CK(hipMemset(base, kCanary, n + 2 * kGuard));
        if (n && fill != kCanary) CK(hipMemset(base + kGuard, fill, n));
    }
    Dev(const Dev&) = delete;
    ~Dev() { CK(hipFree(base)); }
    uint8_t* p() const { return base + kGuard; }
    void put(const void* h) { if (n) CK(hipMemcpy(p(), h, n, hipMemcpyHostToDevice)); }
    std::vector<uint8_t> get(const char* what, const char* name) const
    {
        std::vector<uint8_t> h(n + 2 * kGuard);
        CK(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kGuard; i++) {
            if (h[i] != kCanary) mismatch(what, name, i, h[i], kCanary);
            if (h[kGuard + n + i] != kCanary) mismatch(what, name, kGuard + n + i, h[kGuard + n + i], kCanary);
        }
        return std::vector<uint8_t>(h.begin() + kGuard, h.begin() + kGuard + n);
    }
};

// the rule of the frame layer, restated: a block is stored raw when it did not shrink below its input; a 1-byte block never is
bool model_raw(uint32_t n, uint32_t cs) { return n != 1u && (cs == 0u || cs >= n); }
uint64_t model_record(uint32_t n, uint32_t cs) { return 4ull + (model_raw(n, cs) ? n : cs); }

struct Chunk { std::vector<uint32_t> sizes; uint32_t last; };

void compare_state(const Dev& d_state, uint64_t cursor, bool overflow, uint64_t raw, const char* name)
{
    const std::vector<uint8_t> r = d_state.get("state canary", name);
    uint64_t st[4];
    memcpy(st, r.data(), sizeof st);
    if (st[0] != cursor) mismatch("cursor", name, 0, st[0], cursor);
    if ((st[1] != 0) != overflow) mismatch("overflow flag", name, 0, st[1], overflow);
    if (st[2] != raw) mismatch("raw records", name, 0, st[2], raw);
    if (st[3] != 0) mismatch("reserved word", name, 0, st[3], 0);
}

// the scan alone, launch after launch on one state: offsets are absolute positions, whatever the start
void scan_case(const std::vector<Chunk>& chunks, uint32_t blockSize, uint64_t start, uint64_t limit, const char* name)
{
    Dev d_state(32, 0);
    const uint64_t init[4] = { start, 0, 0, 0 };
    d_state.put(init);
    uint64_t cursor = start, raw = 0;
    bool overflow = false;
    for (const Chunk& c : chunks) {
        const uint32_t nb = (uint32_t)c.sizes.size();
        std::vector<uint64_t> want(nb);
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t n = b + 1 == nb ? c.last : blockSize;
            want[b] = cursor; cursor += model_record(n, c.sizes[b]); raw += model_raw(n, c.sizes[b]);
        }
        overflow = overflow || cursor > limit;
        Dev d_sizes(4 * (size_t)nb), d_offsets(8 * (size_t)nb);
        d_sizes.put(c.sizes.data());
        hipLaunchKernelGGL(lz_frame_scan_kernel, dim3(1), dim3(1024), 0, 0, (const u32*)d_sizes.p(), (u64*)d_offsets.p(), nb, blockSize, c.last,
                           (LzFrameState*)d_state.p(), limit);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        const std::vector<uint8_t> got = d_offsets.get("offsets canary", name);
        for (uint32_t b = 0; b < nb; b++) {
            uint64_t v;
            memcpy(&v, got.data() + 8 * (size_t)b, 8);
            if (v != want[b]) { mismatch("offsets", name, b, v, want[b]); break; }
        }
        compare_state(d_state, cursor, overflow, raw, name);
    }
    g_cases++;
}

// scan + gather, chunk after chunk into one destination.  Every non-raw size is at most `stride`; a chunk's input has
// (nb - 1) * blockSize + last bytes, all a raw record reads.  Returns the frame's size without a limit.
uint64_t frame_case(const std::vector<Chunk>& chunks, size_t stride, uint32_t blockSize, uint64_t start, uint64_t limit, const char* name)
{
    uint64_t total = start;
    for (const Chunk& c : chunks)
        for (size_t b = 0; b < c.sizes.size(); b++) total += model_record(b + 1 == c.sizes.size() ? c.last : blockSize, c.sizes[b]);
    std::vector<uint8_t> frame((size_t)total, kCanary);
    Dev d_dst((size_t)total), d_state(32, 0);
    const uint64_t init[4] = { start, 0, 0, 0 };
    d_state.put(init);
    uint64_t cursor = start, raw = 0;
    bool overflow = false;
    for (const Chunk& c : chunks) {
        const uint32_t nb = (uint32_t)c.sizes.size();
        std::vector<uint8_t> slots((size_t)nb * stride), in((size_t)(nb - 1) * blockSize + c.last);
        for (auto& v : slots) v = (uint8_t)(rnd() | 1u);         // (odd bytes in the slots, even ones in the input: the source shows in every byte)
        for (auto& v : in) v = (uint8_t)(rnd() & ~1u);
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t n = b + 1 == nb ? c.last : blockSize, cs = c.sizes[b];
            const bool r = model_raw(n, cs);
            const uint32_t len = r ? n : cs, word = r ? (n | 0x80000000u) : cs;
            if (!r && len > stride) { fprintf(stderr, "frame_pack_kernels: a case reads outside its slot\n"); exit(2); }
            if (n == 1u && r) { fprintf(stderr, "frame_pack_kernels: the model stores a 1-byte block raw\n"); exit(2); }
            if (cursor + 4 + len <= limit) {
                uint8_t* out = frame.data() + cursor;
                out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
                if (len) memcpy(out + 4, r ? in.data() + (size_t)b * blockSize : slots.data() + (size_t)b * stride, len);
            }
            cursor += 4ull + len; raw += r;
        }
        overflow = overflow || cursor > limit;
        Dev d_sizes(4 * (size_t)nb), d_offsets(8 * (size_t)nb), d_slots(slots.size()), d_in(in.size());
        d_sizes.put(c.sizes.data()); d_slots.put(slots.data()); d_in.put(in.data());
        lz_frame_pack_launch(d_in.p(), d_slots.p(), stride, (const u32*)d_sizes.p(), (u64*)d_offsets.p(), d_dst.p(), nb, blockSize, c.last,
                             (LzFrameState*)d_state.p(), limit, 0);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        if (d_slots.get("slots canary", name) != slots) mismatch("the slots changed", name, 0, 0, 0);
        if (d_in.get("input canary", name) != in) mismatch("the input changed", name, 0, 0, 0);
        (void)d_offsets.get("offsets canary", name);
        compare_state(d_state, cursor, overflow, raw, name);
    }
    const std::vector<uint8_t> got = d_dst.get("destination canary", name);
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != frame[i]) { mismatch(i >= limit ? "a byte at or behind the limit changed" : "frame bytes", name, i, got[i], frame[i]); break; }
    g_cases++;
    return total;
}

Chunk edge_chunk(uint32_t nb, uint32_t blockSize, uint32_t last, int rep)
{
    Chunk c; c.last = last; c.sizes.resize(nb);
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t n = b + 1 == nb ? last : blockSize;
        const uint32_t pick = nb <= 7 ? (b + (uint32_t)rep) % 6u : rnd() % 6u;
        const uint32_t choice[6] = { 0u, 1u, n >= 2u ? n - 2u : 0u, n - 1u, n, n + 5u };
        c.sizes[b] = choice[pick];
    }
    return c;
}
}  // namespace

int main()
{
    int dev = 0;
    CK(hipGetDevice(&dev));
    const uint32_t blockSize = 4099;
    const size_t stride = 4111;                                  // odd, and at least n - 1: a block that shrank by one byte fits its slot
    static const uint32_t lasts[] = { 1, 2, 4099 };
    // ---- the scan alone: three launches on one cursor; more than 1024 blocks; a start above 2^32 ----
    static const uint32_t scanBlocks[] = { 1, 2, 63, 1023, 1024, 1025, 2049, 5000 };
    for (uint32_t nb : scanBlocks)
        for (uint32_t last : lasts) {
            std::vector<Chunk> chunks = { edge_chunk(nb, blockSize, blockSize, 0), edge_chunk(nb / 2 + 1, blockSize, blockSize, 1), edge_chunk(nb, blockSize, last, 2) };
            scan_case(chunks, blockSize, 7, kNoLimit, "scan from 7");
            scan_case(chunks, blockSize, (5ull << 32) + 11, kNoLimit, "scan from above 2^32");
            scan_case(chunks, blockSize, (5ull << 32) + 11, (5ull << 32) + 11 + 3ull * blockSize, "scan from above 2^32 with a limit");
        }
    {   // a chunk total above 2^32: the running sums are 64-bit
        Chunk big; big.last = 0x7FFFFFF0u; big.sizes.assign(5, 0u);
        scan_case({ big, big }, 0x7FFFFFF0u, 15, kNoLimit, "chunk totals above 2^32");
    }
    // ---- scan + gather: three chunks on one cursor, starts on every residue mod 16, the raw rule on its edges, n = 1 ----
    static const uint32_t packBlocks[] = { 1, 7, 1025, 2049 };
    for (uint32_t start = 0; start < 16; start++) {
        const uint32_t last = lasts[start % 3];
        std::vector<Chunk> chunks = { edge_chunk(7, blockSize, blockSize, (int)start), edge_chunk(1, blockSize, blockSize, (int)start + 1), edge_chunk(7, blockSize, last, (int)start + 2) };
        frame_case(chunks, stride, blockSize, start, kNoLimit, "three chunks, start on a residue");
    }
    for (uint32_t last : lasts)
        for (uint32_t nb : packBlocks) {
            std::vector<Chunk> chunks = { edge_chunk(nb, blockSize, blockSize, 0), edge_chunk(3, blockSize, blockSize, 1), edge_chunk(nb, blockSize, last, 2) };
            frame_case(chunks, stride, blockSize, 15, kNoLimit, "three chunks");
        }
    {   // lengths around the 16-byte lane copy and the 4096-byte pass, compressed form
        static const uint32_t edge[] = { 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 4098 };
        for (int rep = 0; rep < 16; rep++) {
            Chunk c; c.last = blockSize;
            for (uint32_t e : edge) c.sizes.push_back(e);
            c.sizes.push_back(edge[rep % 11]);
            frame_case({ c }, stride, blockSize, 7 + (uint64_t)rep, kNoLimit, "lane-copy edges");
        }
    }
    // ---- the limit: on a record's end, one byte before it, inside the first record; in the first, second and third chunk ----
    for (int rep = 0; rep < 4; rep++) {
        std::vector<Chunk> chunks = { edge_chunk(5, blockSize, blockSize, rep), edge_chunk(4, blockSize, blockSize, rep + 1), edge_chunk(6, blockSize, rep & 1 ? 1u : 777u, rep + 2) };
        const uint64_t start = 7 + (uint64_t)rep;
        std::vector<uint64_t> ends;
        uint64_t at = start;
        for (const Chunk& c : chunks)
            for (size_t b = 0; b < c.sizes.size(); b++) { at += model_record(b + 1 == c.sizes.size() ? c.last : blockSize, c.sizes[b]); ends.push_back(at); }
        const uint64_t total = frame_case(chunks, stride, blockSize, start, kNoLimit, "no limit");
        if (total != ends.back()) mismatch("the model's total", "limit cases", 0, total, ends.back());
        frame_case(chunks, stride, blockSize, start, total, "limit = the frame's end");
        frame_case(chunks, stride, blockSize, start, total - 1, "limit one byte before the last record's end");
        for (size_t r : { (size_t)0, (size_t)2, (size_t)4, (size_t)5, (size_t)8, (size_t)9, (size_t)13 }) {
            frame_case(chunks, stride, blockSize, start, ends[r], "limit on a record's end");
            frame_case(chunks, stride, blockSize, start, ends[r] - 1, "limit one byte before a record's end");
            frame_case(chunks, stride, blockSize, start, ends[r] + 1, "limit one byte behind a record's end");
        }
        frame_case(chunks, stride, blockSize, start, start + 3, "limit inside the first record's word");
        frame_case(chunks, stride, blockSize, start, start, "limit at the start");
        frame_case(chunks, stride, blockSize, start, 0, "limit 0, in front of the start");
    }
    printf("cases: %d mismatches: %d\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
