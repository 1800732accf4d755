// tests/frames_pack_kernels.hip — TEST INFRASTRUCTURE: lz_frames_scan_kernel, lz_frames_gather_kernel, lz_frames_finish_kernel and
// lz_xxh32_frames_kernel (lizard_amd/csrc/lz_frames_pack.h) on their own, against a sequential host model, on synthetic tables.
// LizardGPU_compressFrames_device reaches these kernels only with the sizes real compressors produce, whole 128 KiB blocks and the
// capacities its bound allows.  Here:
//   scan + gather + finish: chunks of 1, 63, 64, 65, 1023, 1024, 1025 and 2049 blocks; frame borders behind the first block, in front of
//     the last, behind every block, nowhere, and at random; frames without blocks and entries that are not live between the others in
//     the table; two chunks in succession over one table, so that cursors carry and a frame straddles the chunk border; blocks of 1 to
//     700 bytes at odd addresses whose records are raw or compressed to 1 .. 300 bytes, so lengths are no multiples of 16 and
//     positions are odd; frames whose limit falls on a record's end, inside a record, and on the frame's end.  The flag rises or
//     not, nothing at or behind a limit changes, the records in front of it are whole.  All destinations lie in ONE buffer that is
//     compared whole with the model's image, canary gaps between the frames included.
//   XXH32: every length 0 .. 48, 1023, 1024, 1025 and 65537 at source addresses 0, 1, 2, 3 bytes off a 16-byte boundary, in batches of
//     1, 15, 16, 17 and 65 frames of unequal length (partial waves, partial groups of four lanes), some entries not live or without the
//     checksum flag, against Lizard_XXH32 of lizard_amd/csrc/lizard_xxhash.c compiled into the program.
// 64-byte canaries surround every buffer.  Every HIP call is checked; the program stops at the first error.
//   hipcc -O2 --offload-arch=gfx950 tests/frames_pack_kernels.hip lizard_amd/csrc/lizard_xxhash.c -o tests/frames_pack_kernels
//   prints "cases: N mismatches: 0", exit 0
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lizard_amd/csrc/lz_frames_pack.h"

extern "C" unsigned int Lizard_XXH32(const void* input, size_t length, unsigned int seed);

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "frames_pack_kernels: %s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

namespace {
const size_t kGuard = 64;
const uint8_t kCanary = 0xC3;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
int g_cases, g_bad;

void mismatch(const char* what, const char* name, uint64_t at, uint64_t got, uint64_t want)
{
    if (g_bad++ < 20) fprintf(stderr, "frames_pack_kernels: %s: %s: at %llu got %llu, want %llu\n", name, what,
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
enum Limit { FITS, ON_A_RECORD_END, INSIDE_A_RECORD };

struct Block { uint32_t n, cs, frame; };

// The blocks of all chunks in order, dealt to frames by `layout`; a frame border may fall on the chunk border or not (RANDOM_RUNS
// and ONE_FRAME straddle it).  Between two frames that have blocks the table holds an entry without blocks or one that is not live.
std::vector<Block> make_blocks(size_t total, Layout layout, uint32_t* nFrames)
{
    std::vector<Block> b(total);
    uint32_t f = 0, left = 0;
    for (size_t i = 0; i < total; i++) {
        bool border = false;
        switch (layout) {
        case ONE_FRAME: break;
        case EVERY_BLOCK: border = i > 0; break;
        case FIRST_AND_LAST: border = i == 1 || (i + 1 == total && i > 1); break;
        case RANDOM_RUNS: if (i > 0 && left == 0) border = true; break;
        }
        if (border) f += 1 + (rnd() % 3u == 0 ? 1 + rnd() % 2u : 0);      // skip one or two table entries now and then
        if (layout == RANDOM_RUNS && (i == 0 || border)) left = rnd() % 4u ? rnd() % 5u : rnd() % 700u;
        else if (left) left--;
        const uint32_t n = rnd() % 8u == 0 ? 1u : 1u + rnd() % 700u;
        const uint32_t pick = rnd() % 8u;
        uint32_t cs = pick == 0 ? 0u : pick == 1 ? n : pick == 2 ? n + 3u : 1u + rnd() % 300u;      // raw: 0, n, above n; or compressed
        if (n == 1u) cs = 1u + rnd() % 6u;
        b[i].n = n; b[i].cs = cs; b[i].frame = f;
    }
    *nFrames = f + 2;                                            // (and one entry without blocks behind the last)
    return b;
}

void frames_case(const std::vector<uint32_t>& chunkBlocks, Layout layout, Limit limitKind, const char* name)
{
    const size_t stride = 307;                                   // odd, and every compressed size fits
    size_t total = 0;
    for (uint32_t q : chunkBlocks) total += q;
    uint32_t nFrames = 0;
    const std::vector<Block> blocks = make_blocks(total, layout, &nFrames);
    // the frames: header length 7 .. 15, a place at an odd distance behind the one before, a limit, a hash to be written
    std::vector<LzFramesEntry> frames(nFrames);
    std::vector<uint64_t> need(nFrames, 0), place(nFrames, 0);
    std::vector<std::vector<uint64_t>> ends(nFrames);
    memset(frames.data(), 0, nFrames * sizeof(LzFramesEntry));
    for (const Block& b : blocks) {
        const uint64_t rec = 4ull + (model_raw(b.n, b.cs) ? b.n : b.cs);
        need[b.frame] += rec; ends[b.frame].push_back(need[b.frame]);
    }
    uint64_t dstBytes = 0;
    for (uint32_t f = 0; f < nFrames; f++) {
        LzFramesEntry& e = frames[f];
        const bool live = !ends[f].empty() || rnd() % 2u;
        if (!live) continue;                                     // dst 0, flags 0: the kernels must not touch it
        e.headerBytes = 7u + rnd() % 9u;
        for (uint32_t i = 0; i < e.headerBytes; i++) e.header[i] = (uint8_t)(0x40u + i + f);
        e.flags = LZK_FRAMES_LIVE | (rnd() % 2u ? LZK_FRAMES_CHECKSUM : 0u);
        e.hash = rnd();
        e.cursor = e.headerBytes;
        const uint64_t tail = e.flags & LZK_FRAMES_CHECKSUM ? 8 : 4;
        uint64_t limit = e.headerBytes + need[f];
        if (limitKind != FITS && !ends[f].empty() && f % 3u != 0) {
            const size_t r = rnd() % ends[f].size();
            limit = e.headerBytes + ends[f][r] - (limitKind == INSIDE_A_RECORD ? 1u + rnd() % 4u : 0u);
        }
        e.limit = limit;
        place[f] = dstBytes + 1 + rnd() % 15u;
        dstBytes = place[f] + e.headerBytes + need[f] + tail + kGuard;      // room for the whole frame whatever its limit: a kernel that ignored the limit is caught by the comparison
    }
    Dev d_dst(dstBytes);
    std::vector<uint8_t> image(dstBytes, kCanary);
    for (uint32_t f = 0; f < nFrames; f++) if (frames[f].flags) frames[f].dst = (uint64_t)(uintptr_t)(d_dst.p() + place[f]);
    Dev d_frames(nFrames * sizeof(LzFramesEntry));
    d_frames.put(frames.data());
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
            LzFramesEntry& e = frames[k.frame];
            const bool r = model_raw(k.n, k.cs);
            const uint32_t len = r ? k.n : k.cs, word = r ? (k.n | 0x80000000u) : k.cs;
            if (!r && len > stride) { fprintf(stderr, "frames_pack_kernels: a case reads outside its slot\n"); exit(2); }
            sizes[b] = k.cs; blkSizes[b] = k.n; blkFrames[b] = k.frame;
            want[b] = e.cursor;
            if (e.cursor + 4 + len <= e.limit) {
                uint8_t* out = image.data() + place[k.frame] + e.cursor;
                out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
                memcpy(out + 4, r ? in.data() + blkOffsets[b] : slots.data() + (size_t)b * stride, len);
            }
            e.cursor += 4ull + len; e.rawRecords += r;
            if (e.cursor > e.limit) e.overflow = 1;
        }
        Dev d_sizes(4 * (size_t)q), d_blkSizes(4 * (size_t)q), d_blkFrames(4 * (size_t)q), d_blkOffsets(8 * (size_t)q), d_offsets(8 * (size_t)q);
        Dev d_slots(slots.size()), d_in(in.size());
        d_sizes.put(sizes.data()); d_blkSizes.put(blkSizes.data()); d_blkFrames.put(blkFrames.data()); d_blkOffsets.put(blkOffsets.data());
        d_slots.put(slots.data()); d_in.put(in.data());
        lz_frames_pack_launch(d_in.p(), (const u64*)d_blkOffsets.p(), (const u32*)d_blkSizes.p(), (const u32*)d_blkFrames.p(), d_slots.p(), stride,
                              (const u32*)d_sizes.p(), (u64*)d_offsets.p(), q, (LzFramesEntry*)d_frames.p(), 0);
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
        const std::vector<uint8_t> tab = d_frames.get("frame table canary", name);
        if (memcmp(tab.data(), frames.data(), tab.size())) {
            for (uint32_t f = 0; f < nFrames; f++) {
                LzFramesEntry got;
                memcpy(&got, tab.data() + f * sizeof got, sizeof got);
                if (got.cursor != frames[f].cursor) { mismatch("a frame's cursor", name, f, got.cursor, frames[f].cursor); break; }
                if (got.overflow != frames[f].overflow) { mismatch("a frame's overflow flag", name, f, got.overflow, frames[f].overflow); break; }
                if (got.rawRecords != frames[f].rawRecords) { mismatch("a frame's raw records", name, f, got.rawRecords, frames[f].rawRecords); break; }
                if (memcmp(&got, &frames[f], sizeof got)) { mismatch("a frame's entry", name, f, 0, 0); break; }
            }
        }
        first += q;
    }
    // heads, tails and result records
    std::vector<LzFramesResult> results(nFrames);
    for (uint32_t f = 0; f < nFrames; f++) {
        const LzFramesEntry& e = frames[f];
        LzFramesResult r = { 0, 0, 0 };
        if (e.flags) {
            uint8_t* at = image.data() + place[f];
            memcpy(at, e.header, e.headerBytes);
            r.rawRecords = e.rawRecords;
            if (e.overflow) r.size = LZK_FRAMES_OVERFLOW;
            else {
                memset(at + e.cursor, 0, 4); r.size = e.cursor + 4;
                if (e.flags & LZK_FRAMES_CHECKSUM) { for (int i = 0; i < 4; i++) at[e.cursor + 4 + i] = (uint8_t)(e.hash >> (8 * i)); r.size += 4; }
            }
        }
        results[f] = r;
    }
    Dev d_results(nFrames * sizeof(LzFramesResult));
    lz_frames_finish_launch((const LzFramesEntry*)d_frames.p(), (LzFramesResult*)d_results.p(), nFrames, 0);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    const std::vector<uint8_t> res = d_results.get("result records canary", name);
    for (uint32_t f = 0; f < nFrames; f++)
        if (memcmp(res.data() + f * sizeof(LzFramesResult), &results[f], sizeof(LzFramesResult))) { mismatch("a frame's result record", name, f, 0, results[f].size); break; }
    const std::vector<uint8_t> got = d_dst.get("destination canary", name);
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != image[i]) { mismatch("destination bytes (a frame, or a gap between frames)", name, i, got[i], image[i]); break; }
    g_cases++;
}

// nFrames entries; entry i hashes lens[i] bytes that start aligns[i] bytes off a 16-byte boundary.  mixed: about a quarter of the
// entries are not live or carry no checksum flag, and their hash must stay as it is
void hash_case(const std::vector<uint32_t>& lens, const std::vector<uint32_t>& aligns, bool mixed, const char* name)
{
    const uint32_t nFrames = (uint32_t)lens.size();
    std::vector<LzFramesEntry> frames(nFrames);
    std::vector<uint64_t> at(nFrames);
    memset(frames.data(), 0, nFrames * sizeof(LzFramesEntry));
    uint64_t bytes = 0;
    for (uint32_t f = 0; f < nFrames; f++) { bytes = ((bytes + 15) & ~15ull) + aligns[f]; at[f] = bytes; bytes += lens[f]; }
    std::vector<uint8_t> in(bytes + 16);
    for (auto& v : in) v = (uint8_t)rnd();
    Dev d_in(in.size());
    d_in.put(in.data());
    if (((uintptr_t)d_in.p() & 15u) != 0) { fprintf(stderr, "frames_pack_kernels: the input buffer is not 16-byte aligned\n"); exit(2); }
    for (uint32_t f = 0; f < nFrames; f++) {
        LzFramesEntry& e = frames[f];
        const uint32_t kind = mixed ? rnd() % 8u : 2u;           // 0: not live, 1: live without a checksum
        e.flags = kind == 0 ? 0u : kind == 1 ? LZK_FRAMES_LIVE : LZK_FRAMES_LIVE | LZK_FRAMES_CHECKSUM;
        e.src = (uint64_t)(uintptr_t)(d_in.p() + at[f]); e.srcSize = lens[f];
        e.hash = 0xDEADBEEFu; e.cursor = f; e.limit = ~0ull;
    }
    Dev d_frames(nFrames * sizeof(LzFramesEntry));
    d_frames.put(frames.data());
    lz_frames_hash_launch((LzFramesEntry*)d_frames.p(), nFrames, 0);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (d_in.get("input canary", name) != in) mismatch("the input changed", name, 0, 0, 0);
    const std::vector<uint8_t> tab = d_frames.get("frame table canary", name);
    for (uint32_t f = 0; f < nFrames; f++) {
        LzFramesEntry got;
        memcpy(&got, tab.data() + f * sizeof got, sizeof got);
        if (frames[f].flags == (LZK_FRAMES_LIVE | LZK_FRAMES_CHECKSUM)) frames[f].hash = Lizard_XXH32(in.data() + at[f], lens[f], 0);
        if (got.hash != frames[f].hash) mismatch("XXH32 (at: 1000 x length + offset from 16)", name, 1000ull * lens[f] + aligns[f], got.hash, frames[f].hash);
        else if (memcmp(&got, &frames[f], sizeof got)) mismatch("a frame's entry", name, f, 0, 0);
    }
    g_cases++;
}
}  // namespace

int main()
{
    int dev = 0;
    CK(hipGetDevice(&dev));
    // ---- scan + gather + finish ----
    static const uint32_t chunks[] = { 1, 63, 64, 65, 1023, 1024, 1025, 2049 };
    static const Layout layouts[] = { ONE_FRAME, EVERY_BLOCK, FIRST_AND_LAST, RANDOM_RUNS };
    static const char* const layoutNames[] = { "one frame for all", "every block its own frame", "borders behind the first and in front of the last block", "random runs" };
    for (uint32_t q : chunks)
        for (int l = 0; l < 4; l++) {
            frames_case({ q }, layouts[l], FITS, layoutNames[l]);
            frames_case({ q, q / 2u + 1u }, layouts[l], FITS, layoutNames[l]);       // two chunks over one table: cursors carry
        }
    for (int rep = 0; rep < 6; rep++)
        for (int l = 0; l < 4; l++) {
            const uint32_t q = chunks[(rep + l) % 8];
            frames_case({ q, 65u }, layouts[l], ON_A_RECORD_END, "limits on a record's end");
            frames_case({ 7u, q }, layouts[l], INSIDE_A_RECORD, "limits inside a record");
        }
    // ---- XXH32: every (length, offset) once, dealt to batches of 1, 15, 16, 17 and 65 frames ----
    std::vector<uint32_t> lens, aligns;
    for (uint32_t a = 0; a < 4; a++) {
        for (uint32_t n = 0; n <= 48; n++) { lens.push_back(n); aligns.push_back(a); }
        for (uint32_t n : { 1023u, 1024u, 1025u, 65537u }) { lens.push_back(n); aligns.push_back(a); }
    }
    for (size_t i = lens.size(); i > 1; i--) { const size_t k = rnd() % i; std::swap(lens[i - 1], lens[k]); std::swap(aligns[i - 1], aligns[k]); }
    static const size_t batch[] = { 1, 15, 16, 17, 65 };
    for (size_t i = 0, b = 0; i < lens.size(); b++) {
        const size_t n = std::min(batch[b % 5], lens.size() - i);
        hash_case(std::vector<uint32_t>(lens.begin() + i, lens.begin() + i + n), std::vector<uint32_t>(aligns.begin() + i, aligns.begin() + i + n), n > 2, "a batch of hashes");
        i += n;
    }
    hash_case(lens, aligns, false, "all lengths and offsets in one batch, every entry hashed");
    printf("cases: %d mismatches: %d\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
