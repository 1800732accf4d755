// tests/stream_pack_kernels.hip — TEST INFRASTRUCTURE: lz_stream_scan_kernel, lz_frames_gather_kernel as the stream entry launches it and
// lz_stream_finish_kernel (lizard_amd/csrc/lz_stream_pack.h) on their own, against a sequential host model, on synthetic tables.
// LizardGPU_compressStream_device reaches these kernels only with the sizes real compressors produce and whole 128 KiB blocks.  Here:
//   streams of 1, 2 and 1 025 blocks (the last: more than one block per scan thread) in one chunk, and of two chunks (1 025 + 65, 7 + 64)
//     so that the carry word carries and a frame straddles the chunk border; frame borders nowhere, behind every block, behind the
//     first and in front of the last block, and at random, with frames WITHOUT blocks between the others, two of them next to each
//     other, in front of the first and behind the last; blocks of 1 to 700 bytes at odd addresses whose records are raw or compressed
//     to 1 .. 300 bytes; prefixes of 0 .. 100 bytes and one of 1 000; headers of 7 .. 15 bytes; tails of 4 and 8 bytes;
//   capacities: exactly the stream, one byte less, somewhere inside.  The flag rises or not; below its size the stream leaves every
//     byte at or behind the capacity alone and writes no head or tail; the destination is compared whole with the model's image.
// After every chunk the state (carry, overflow, raw records), the positions and the stream table are compared; after the finish
// the result record and the frame offsets.  64-byte canaries surround every buffer.  Every HIP call is checked; the program stops at
// the first error.
//   hipcc -O2 --offload-arch=gfx950 tests/stream_pack_kernels.hip -o tests/stream_pack_kernels
//   prints "cases: N mismatches: 0", exit 0
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lizard_amd/csrc/lz_stream_pack.h"

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "stream_pack_kernels: %s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

namespace {
const size_t kGuard = 64;
const uint8_t kCanary = 0xC3;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
int g_cases, g_bad;

void mismatch(const char* what, const char* name, uint64_t at, uint64_t got, uint64_t want)
{
    if (g_bad++ < 20) fprintf(stderr, "stream_pack_kernels: %s: %s: at %llu got %llu, want %llu\n", name, what,
                              (unsigned long long)at, (unsigned long long)got, (unsigned long long)want);
}

// a device buffer of n bytes between two canaries
struct Dev {
    uint8_t* base = nullptr; size_t n = 0;
    explicit Dev(size_t bytes) : n(bytes)
    {
        CK(hipMalloc((void**)&base, n + 2 * kGuard));
        CK(hipMemset(base, kCanary, n + 2 * kGuard));
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

enum Layout { ONE_FRAME, EVERY_BLOCK, FIRST_AND_LAST, RANDOM_RUNS };
enum Capacity { EXACT, ONE_BELOW, INSIDE };

struct Block { uint32_t n, cs, frame; };

// The blocks of all chunks in order, dealt to frames by `layout`.  Frame 0 has no blocks; between two frames that have some the table
// holds none, one or two frames without; two more stand behind the last.
std::vector<Block> make_blocks(size_t total, Layout layout, uint32_t* nFrames)
{
    std::vector<Block> b(total);
    uint32_t f = 1, left = 0;
    for (size_t i = 0; i < total; i++) {
        bool border = false;
        switch (layout) {
        case ONE_FRAME: break;
        case EVERY_BLOCK: border = i > 0; break;
        case FIRST_AND_LAST: border = i == 1 || (i + 1 == total && i > 1); break;
        case RANDOM_RUNS: if (i > 0 && left == 0) border = true; break;
        }
        if (border) f += 1 + (rnd() % 3u == 0 ? 1 + rnd() % 2u : 0);
        if (layout == RANDOM_RUNS && (i == 0 || border)) left = rnd() % 4u ? rnd() % 5u : rnd() % 700u;
        else if (left) left--;
        const uint32_t n = rnd() % 8u == 0 ? 1u : 1u + rnd() % 700u;
        const uint32_t pick = rnd() % 8u;
        uint32_t cs = pick == 0 ? 0u : pick == 1 ? n : pick == 2 ? n + 3u : 1u + rnd() % 300u;      // raw: 0, n, above n; or compressed
        if (n == 1u) cs = 1u + rnd() % 6u;
        b[i].n = n; b[i].cs = cs; b[i].frame = f;
    }
    *nFrames = f + 3;
    return b;
}

void stream_case(const std::vector<uint32_t>& chunkBlocks, Layout layout, Capacity capKind, const char* name)
{
    const size_t stride = 307;                                   // odd, and every compressed size fits
    size_t total = 0;
    for (uint32_t q : chunkBlocks) total += q;
    uint32_t F = 0;
    const std::vector<Block> blocks = make_blocks(total, layout, &F);
    // the two tables as the host file fills them
    std::vector<LzFramesEntry> frames(F);
    std::vector<LzStreamEntry> entries(F);
    memset(frames.data(), 0, F * sizeof(LzFramesEntry));
    memset(entries.data(), 0, F * sizeof(LzStreamEntry));
    for (uint32_t f = 0; f < F; f++) { entries[f].firstBlock = entries[f].lastBlock = 0xFFFFFFFFu; }
    uint64_t records = 0;
    for (size_t i = 0; i < total; i++) {
        const Block& b = blocks[i];
        if (entries[b.frame].firstBlock == 0xFFFFFFFFu) entries[b.frame].firstBlock = (uint32_t)i;
        entries[b.frame].lastBlock = (uint32_t)i;
        frames[b.frame].nBlocks++;
        records += 4ull + (model_raw(b.n, b.cs) ? b.n : b.cs);
    }
    std::vector<uint8_t> blob;
    uint64_t fixed = 0;
    for (uint32_t f = 0; f < F; f++) {
        LzFramesEntry& e = frames[f];
        LzStreamEntry& s = entries[f];
        e.headerBytes = 7u + rnd() % 9u;
        for (uint32_t i = 0; i < e.headerBytes; i++) e.header[i] = (uint8_t)(0x40u + i + f);
        e.flags = LZK_FRAMES_LIVE | (rnd() % 2u ? LZK_FRAMES_CHECKSUM : 0u);
        e.hash = rnd();
        s.prefixOff = blob.size();
        s.prefixBytes = f == 2 ? 1000u : rnd() % 3u == 0 ? 0u : rnd() % 101u;
        for (uint64_t i = 0; i < s.prefixBytes; i++) blob.push_back((uint8_t)(0x80u | rnd()));
        fixed += s.prefixBytes + e.headerBytes;
        s.fixed = fixed;
        s.tailBytes = e.flags & LZK_FRAMES_CHECKSUM ? 8u : 4u;
        fixed += s.tailBytes;
    }
    uint32_t next = F;
    for (uint32_t f = F; f-- > 0;) {
        entries[f].nextAfter = next;
        if (frames[f].nBlocks) next = f;
        entries[f].nextSelf = next;
    }
    blob.push_back(0);
    const uint64_t fixedTotal = fixed, size = fixedTotal + records;
    const uint64_t capacity = capKind == EXACT ? size : capKind == ONE_BELOW ? size - 1 : rnd() % size;
    Dev d_dst(size + 40);                                        // room behind every capacity: a kernel that ignored it is caught by the comparison
    std::vector<uint8_t> image(size + 40, kCanary);
    for (uint32_t f = 0; f < F; f++) { frames[f].dst = (uint64_t)(uintptr_t)d_dst.p(); frames[f].limit = capacity; }
    LzStreamState state = { 0, 0, 0 };
    Dev d_frames(F * sizeof(LzFramesEntry)), d_entries(F * sizeof(LzStreamEntry)), d_blob(blob.size()), d_state(sizeof state);
    d_frames.put(frames.data()); d_entries.put(entries.data()); d_blob.put(blob.data()); d_state.put(&state);
    // chunk after chunk
    size_t first = 0;
    for (uint32_t q : chunkBlocks) {
        std::vector<uint8_t> slots((size_t)q * stride);
        std::vector<uint32_t> sizes(q), blkSizes(q), blkFrames(q);
        std::vector<uint64_t> blkOffsets(q), want(q);
        uint64_t inBytes = 3;
        for (uint32_t b = 0; b < q; b++) { blkOffsets[b] = inBytes; inBytes += blocks[first + b].n + rnd() % 3u; }
        std::vector<uint8_t> in(inBytes);
        for (auto& v : slots) v = (uint8_t)(rnd() | 1u);         // (odd bytes in the slots, even ones in the input: the source shows in every byte)
        for (auto& v : in) v = (uint8_t)(rnd() & ~1u);
        for (uint32_t b = 0; b < q; b++) {
            const Block& k = blocks[first + b];
            LzStreamEntry& s = entries[k.frame];
            const bool r = model_raw(k.n, k.cs);
            const uint32_t len = r ? k.n : k.cs, word = r ? (k.n | 0x80000000u) : k.cs;
            if (!r && len > stride) { fprintf(stderr, "stream_pack_kernels: a case reads outside its slot\n"); exit(2); }
            sizes[b] = k.cs; blkSizes[b] = k.n; blkFrames[b] = k.frame;
            if (first + b == s.firstBlock) s.before = state.carry;
            want[b] = s.fixed + state.carry;
            if (want[b] + 4 + len <= capacity) {
                uint8_t* out = image.data() + want[b];
                out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
                memcpy(out + 4, r ? in.data() + blkOffsets[b] : slots.data() + (size_t)b * stride, len);
            }
            state.carry += 4ull + len; state.rawRecords += r;
            if (s.fixed + state.carry + (first + b == s.lastBlock ? s.tailBytes : 0u) > capacity) state.overflow = 1;
        }
        Dev d_sizes(4 * (size_t)q), d_blkSizes(4 * (size_t)q), d_blkFrames(4 * (size_t)q), d_blkOffsets(8 * (size_t)q), d_offsets(8 * (size_t)q);
        Dev d_slots(slots.size()), d_in(in.size());
        d_sizes.put(sizes.data()); d_blkSizes.put(blkSizes.data()); d_blkFrames.put(blkFrames.data()); d_blkOffsets.put(blkOffsets.data());
        d_slots.put(slots.data()); d_in.put(in.data());
        lz_stream_pack_launch(d_in.p(), (const u64*)d_blkOffsets.p(), (const u32*)d_blkSizes.p(), (const u32*)d_blkFrames.p(), d_slots.p(), stride,
                              (const u32*)d_sizes.p(), (u64*)d_offsets.p(), q, (u32)first, (const LzFramesEntry*)d_frames.p(), (LzStreamEntry*)d_entries.p(),
                              (LzStreamState*)d_state.p(), capacity, 0);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        if (d_slots.get("slots canary", name) != slots) mismatch("the slots changed", name, 0, 0, 0);
        if (d_in.get("input canary", name) != in) mismatch("the input changed", name, 0, 0, 0);
        const std::vector<uint8_t> offs = d_offsets.get("offsets canary", name);
        for (uint32_t b = 0; b < q; b++) {
            uint64_t v;
            memcpy(&v, offs.data() + 8 * (size_t)b, 8);
            if (v != want[b]) { mismatch("offsets", name, first + b, v, want[b]); break; }
        }
        LzStreamState got;
        memcpy(&got, d_state.get("state canary", name).data(), sizeof got);
        if (got.carry != state.carry) mismatch("the carry", name, first, got.carry, state.carry);
        if (got.overflow != state.overflow) mismatch("the overflow flag", name, first, got.overflow, state.overflow);
        if (got.rawRecords != state.rawRecords) mismatch("the raw records", name, first, got.rawRecords, state.rawRecords);
        const std::vector<uint8_t> tab = d_entries.get("stream table canary", name);
        if (memcmp(tab.data(), entries.data(), tab.size()))
            for (uint32_t f = 0; f < F; f++) {
                LzStreamEntry e;
                memcpy(&e, tab.data() + f * sizeof e, sizeof e);
                if (e.before != entries[f].before) { mismatch("the record bytes in front of a frame", name, f, e.before, entries[f].before); break; }
                if (memcmp(&e, &entries[f], sizeof e)) { mismatch("a frame's stream entry", name, f, 0, 0); break; }
            }
        if (memcmp(d_frames.get("frame table canary", name).data(), frames.data(), F * sizeof(LzFramesEntry))) mismatch("the frame table changed", name, 0, 0, 0);
        first += q;
    }
    // prefixes, heads, tails, offsets and the result record
    const bool over = state.overflow || size > capacity;
    std::vector<uint64_t> offsets(F + 1, 0xC3C3C3C3C3C3C3C3ull);
    LzFramesResult result = { over ? LZK_FRAMES_OVERFLOW : size, state.rawRecords, 0 };
    offsets[F] = size;
    for (uint32_t f = 0; f < F && !over; f++) {
        const LzFramesEntry& e = frames[f];
        const LzStreamEntry& s = entries[f];
        const uint64_t before = s.nextSelf < F ? entries[s.nextSelf].before : state.carry, after = s.nextAfter < F ? entries[s.nextAfter].before : state.carry;
        const uint64_t start = s.fixed - e.headerBytes - s.prefixBytes + before;
        memcpy(image.data() + start, blob.data() + s.prefixOff, s.prefixBytes);
        memcpy(image.data() + start + s.prefixBytes, e.header, e.headerBytes);
        memset(image.data() + s.fixed + after, 0, 4);
        if (s.tailBytes == 8) for (int i = 0; i < 4; i++) image[s.fixed + after + 4 + i] = (uint8_t)(e.hash >> (8 * i));
        offsets[f] = start;
    }
    Dev d_result(sizeof result), d_offs(8 * ((size_t)F + 1));
    lz_stream_finish_launch((const LzFramesEntry*)d_frames.p(), (const LzStreamEntry*)d_entries.p(), d_blob.p(), (const LzStreamState*)d_state.p(), F, fixedTotal,
                            capacity, (LzFramesResult*)d_result.p(), (u64*)d_offs.p(), 0);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (memcmp(d_result.get("result record canary", name).data(), &result, sizeof result)) mismatch("the result record", name, 0, 0, result.size);
    const std::vector<uint8_t> offs = d_offs.get("frame offsets canary", name);
    for (uint32_t f = 0; f <= F; f++) {
        uint64_t v;
        memcpy(&v, offs.data() + 8 * (size_t)f, 8);
        if (v != offsets[f]) { mismatch("a frame's offset", name, f, v, offsets[f]); break; }
    }
    if (!over && (offsets[0] != 0 || image[size] != kCanary)) mismatch("the model's own image", name, 0, offsets[0], 0);
    const std::vector<uint8_t> got = d_dst.get("destination canary", name);
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != image[i]) { mismatch("destination bytes", name, i, got[i], image[i]); break; }
    g_cases++;
}
}  // namespace

int main()
{
    int dev = 0;
    CK(hipGetDevice(&dev));
    static const Layout layouts[] = { ONE_FRAME, EVERY_BLOCK, FIRST_AND_LAST, RANDOM_RUNS };
    static const char* const layoutNames[] = { "one frame for all", "every block its own frame", "borders behind the first and in front of the last block", "random runs" };
    static const Capacity caps[] = { EXACT, ONE_BELOW, INSIDE };
    for (int l = 0; l < 4; l++)
        for (int c = 0; c < 3; c++) {
            for (uint32_t q : { 1u, 2u, 1025u }) stream_case({ q }, layouts[l], caps[c], layoutNames[l]);
            stream_case({ 1025u, 65u }, layouts[l], caps[c], layoutNames[l]);      // two chunks over one carry word
            stream_case({ 7u, 64u }, layouts[l], caps[c], layoutNames[l]);
        }
    printf("cases: %d mismatches: %d\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
