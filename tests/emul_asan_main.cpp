// tests/emul_asan_main.cpp — TEST INFRASTRUCTURE ONLY: the memory footprint of the compress kernels, on the CPU.
//
// A program of its own (tests/test_emulator_asan.py builds and runs it) that drives the product's kernel bodies on the SIMT
// emulator under AddressSanitizer + UndefinedBehaviorSanitizer.  tests/emul/emul_api.cpp is compiled with -DLZ_EMUL_EXACT_AREAS:
// every table, workspace, summary, ring, scratch slot and arena is a heap allocation of exactly the size the product declares.
// Here the source of a case is malloc(n) and its destination malloc(Lizard_compressBound(n)), so a read past the source, a store
// past the bound or past any of the kernel's own areas ends the program with a report.  Every result is also compared byte for
// byte with the oracle compiled into the same program.
//
//   emul_asan_main [huf-case-file]      (the file: huf_stream_inputs.write_case_file; without it the huff0-alone part is left out)
//
// Last line: "cases: N mismatches: M seconds: S"; exit status 0 only with M == 0.
#include <atomic>
#include <chrono>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>
#include "../oracle/lizard_oracle.h"

extern "C" int emul_compress_block(const void* src, int n, void* dst, int level, unsigned seed);
extern "C" int emul_compress_split_ragged(const void* src, int nBlocks, int blockSize, int lastBlockSize, const unsigned* srcSizes, void* dst,
                                          int dstStride, unsigned* sizes, int level, int nProd, int nCons, int activeProd, unsigned seed);
extern "C" int emul_put_stream_huf(const void* stream, int n, void* out, int* huffed, unsigned seed);

namespace {

enum Kind { kNoise = 0, kRun, kText, kNoiseTailRepeat, kKinds };
const char* const kKindName[kKinds] = { "noise", "run", "text", "noise+tail-repeat" };

uint32_t rng_next(uint32_t& s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }

// noise: incompressible (the block is stored raw, the output ends at the bound).  run: one byte value.  text: a sentence over
// and over with a changed byte every few hundred.  noise+tail-repeat: noise whose bytes [n - 56, n - 16) repeat the 40 bytes
// in front of them at distance 44 (short blocks: distance 8) — a match that ends at n - LASTLITERALS.
void fill(uint8_t* d, size_t n, Kind kind, uint32_t salt)
{
    uint32_t s = 0x9E3779B9u ^ (salt * 2654435761u) ^ (uint32_t)n;
    if (!s) s = 1;
    if (kind == kRun) { memset(d, 0x41 + (int)(salt % 7u), n); return; }
    if (kind == kText) {
        static const char sentence[] = "the quick brown fox jumps over the lazy dog; pack my box with five dozen liquor jugs. ";
        for (size_t i = 0; i < n; i++) d[i] = (uint8_t)sentence[i % (sizeof sentence - 1)];
        for (size_t i = rng_next(s) % 300u; i < n; i += 1u + rng_next(s) % 600u) d[i] = (uint8_t)rng_next(s);
        return;
    }
    for (size_t i = 0; i < n; i++) d[i] = (uint8_t)(rng_next(s) >> 11);
    if (kind == kNoiseTailRepeat && n >= 32) {
        const size_t dist = n >= 128 ? 44 : 8, from = n >= 56 + dist ? n - 56 : dist;
        for (size_t i = from; i < n - 16; i++) d[i] = d[i - dist];
    }
}

std::atomic<long> g_cases{0}, g_bad{0};

void mismatch(const char* what, int level, size_t n, int kind, unsigned seed, const char* detail)
{
    g_bad++;
    fprintf(stderr, "MISMATCH %s level %d n %zu data %s seed %u: %s\n", what, level, n, kKindName[kind], seed, detail);
}

struct OneCase { int level; int n; int kind; unsigned seed; };

void run_one(const OneCase& c)
{
    uint8_t* const src = (uint8_t*)malloc((size_t)c.n);                         // exactly n: a read behind the source is a report
    fill(src, (size_t)c.n, (Kind)c.kind, (unsigned)c.n * 4u + (unsigned)c.kind);
    const int bound = lzo_compress_bound(c.n);
    uint8_t* const dst = (uint8_t*)malloc((size_t)bound);                       // exactly the bound
    uint8_t* const want = (uint8_t*)malloc((size_t)bound);
    memset(dst, 0xC3, (size_t)bound);
    const int w = lzo_compress(src, want, c.n, bound, c.level);
    const int r = emul_compress_block(src, c.n, dst, c.level, c.seed);
    g_cases++;
    if (w <= 0) mismatch("block", c.level, (size_t)c.n, c.kind, c.seed, "the oracle refused the case");
    else if (r != w) { char t[96]; snprintf(t, sizeof t, "size %d, oracle %d (bound %d)", r, w, bound); mismatch("block", c.level, (size_t)c.n, c.kind, c.seed, t); }
    else if (r > bound || memcmp(dst, want, (size_t)r)) mismatch("block", c.level, (size_t)c.n, c.kind, c.seed, "bytes differ from the oracle's");
    free(src); free(dst); free(want);
}

const int kLevels[] = { 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 30, 31, 32, 33, 34, 35, 36, 37, 38, 40, 41, 42 };   // every level emul_compress_block dispatches
const int kSmall[] = { 1, 2, 7, 8, 15, 16, 17, 19, 20, 21, 63, 64, 65, 255, 4095, 4096, 4097 };
// one level per kernel family, without and with huff0: fast12, fast18, noChain, hashChain, fastBig, priceFast14, priceFast18
const int kFamily[] = { 10, 30, 11, 31, 12, 33, 13, 34, 20, 40, 21, 41, 22, 42 };
const int kLarge[] = { 65535, 65537, 131071, 131072, 131073, 262145 };

// One seed per table form of the level (emul_api.cpp, exact mode): bit 0 picks global / LDS tables at levels 30 and 21 / 41, bit 1
// the occupancy summary / slot codes at 11 / 31, 20 / 40, 22 / 42 and the 18-bit LDS form at 21 / 41.
std::vector<unsigned> form_seeds(int level)
{
    const int base = level >= 30 ? level - 20 : level;
    if (level == 30 || base == 21) return { 0u, 1u, 2u };
    if (base == 11 || base == 20 || base == 22) return { 0u, 2u };
    return { 0u };
}

void build_block_cases(std::vector<OneCase>& out)
{
    // the long ones first: the worker threads finish together
    for (int i = (int)(sizeof kLarge / sizeof kLarge[0]) - 1; i >= 0; i--) {
        const int n = kLarge[i];
        for (int level : kFamily)
            for (unsigned seed : form_seeds(level))
                for (int kind = 0; kind < kKinds; kind++) out.push_back({ level, n, kind, seed });
    }
    for (int level : kLevels)
        for (int n : kSmall)
            for (unsigned seed = 0; seed < 4; seed++)
                for (int kind = 0; kind < kKinds; kind++) out.push_back({ level, n, kind, seed });
}

// Levels 10 / 30 in the producer / consumer form: dst is nBlocks slots of exactly bound(blockSize), the source exactly the blocks.
void run_split(int level, int nProd, int nCons, int nBlocks, int blockSize, int lastBlockSize, unsigned seed)
{
    const size_t total = (size_t)(nBlocks - 1) * (size_t)blockSize + (size_t)lastBlockSize;
    const int stride = lzo_compress_bound(blockSize);
    uint8_t* const src = (uint8_t*)malloc(total);
    uint8_t* const dst = (uint8_t*)malloc((size_t)nBlocks * (size_t)stride);
    unsigned* const sizes = (unsigned*)malloc(4u * (size_t)nBlocks);
    uint8_t* const want = (uint8_t*)malloc((size_t)stride);
    memset(dst, 0xC3, (size_t)nBlocks * (size_t)stride);
    for (int b = 0; b < nBlocks; b++) {
        sizes[b] = 0xA5A5A5A5u;
        const int n = b == nBlocks - 1 ? lastBlockSize : blockSize;
        fill(src + (size_t)b * (size_t)blockSize, (size_t)n, (Kind)(b % kKinds), (unsigned)b + 17u * seed);   // the kinds mixed block by block
    }
    const int rc = emul_compress_split_ragged(src, nBlocks, blockSize, lastBlockSize, nullptr, dst, stride, sizes, level, nProd, nCons, 0, seed);
    g_cases++;
    char what[64]; snprintf(what, sizeof what, "split %d+%d x%d", nProd, nCons, nBlocks);
    if (rc != 0) mismatch(what, level, (size_t)blockSize, 0, seed, "refused");
    for (int b = 0; rc == 0 && b < nBlocks; b++) {
        const int n = b == nBlocks - 1 ? lastBlockSize : blockSize;
        const int w = lzo_compress(src + (size_t)b * (size_t)blockSize, want, n, stride, level);
        if (w <= 0 || sizes[b] != (unsigned)w || memcmp(dst + (size_t)b * (size_t)stride, want, (size_t)w)) {
            char t[96]; snprintf(t, sizeof t, "block %d: size %u, oracle %d", b, sizes[b], w);
            mismatch(what, level, (size_t)n, b % kKinds, seed, t);
        }
    }
    free(src); free(dst); free(sizes); free(want);
}

uint32_t rd32(FILE* f) { uint8_t b[4]; if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "case file: short read\n"); exit(2); } return b[0] | b[1] << 8 | b[2] << 16 | (uint32_t)b[3] << 24; }

// lz_put_stream_huf alone on the named streams: the output buffer is exactly n + 3 (LE24 n and the raw bytes: the most the stage
// may write), the workspace exactly 4 * LZ_HUF_WS_WORDS (emul_put_stream_huf allocates it so).
void run_huf_streams(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    char magic[4];
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "HUFS", 4)) { fprintf(stderr, "%s: not a stream case file\n", path); exit(2); }
    const uint32_t count = rd32(f);
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t nameLen = rd32(f), n = rd32(f), wantLen = rd32(f), wantHuffed = rd32(f);
        std::string name(nameLen, ' ');
        uint8_t* const data = (uint8_t*)malloc(n);
        uint8_t* const want = (uint8_t*)malloc(wantLen);
        if (fread(&name[0], 1, nameLen, f) != nameLen || fread(data, 1, n, f) != n || fread(want, 1, wantLen, f) != wantLen) { fprintf(stderr, "case file: short read\n"); exit(2); }
        uint8_t* const out = (uint8_t*)malloc((size_t)n + 3u);
        memset(out, 0xC3, (size_t)n + 3u);
        int huffed = -1;
        const int r = emul_put_stream_huf(data, (int)n, out, &huffed, i);
        g_cases++;
        if (r != (int)wantLen || huffed != (int)wantHuffed || (size_t)r > (size_t)n + 3u || memcmp(out, want, wantLen)) {
            char t[128]; snprintf(t, sizeof t, "stream %s: size %d huffed %d, expected %u %u", name.c_str(), r, huffed, wantLen, wantHuffed);
            mismatch("huff0", 0, n, 0, i, t);
        }
        free(data); free(want); free(out);
    }
    fclose(f);
}

}  // namespace

int main(int argc, char** argv)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<OneCase> cases;
    build_block_cases(cases);
    unsigned nThreads = std::thread::hardware_concurrency();
    if (const char* e = getenv("EMUL_ASAN_THREADS")) nThreads = (unsigned)atoi(e);
    if (nThreads < 1) nThreads = 1;
    if (nThreads > 8) nThreads = 8;
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nThreads; t++)
        pool.emplace_back([&] { for (size_t i; (i = next++) < cases.size(); ) run_one(cases[i]); });
    for (auto& t : pool) t.join();
    const long blockCases = g_cases;
    // the split form: every wave is a thread of its own, so these run one after the other.  7 blocks of 65 537 and a ragged last
    // one; 5 blocks of 131 073 (a 1-byte last sub-block in every block).  Seed bit 0: two / three buffers per producer.
    const int waves[3][2] = { { 1, 1 }, { 3, 2 }, { 13, 3 } };
    for (int level : { 10, 30 })
        for (const auto& w : waves)
            for (unsigned seed = 0; seed < 2; seed++) {
                run_split(level, w[0], w[1], 8, 65537, seed ? 1 : 40000, seed);
                run_split(level, w[0], w[1], 5, 131073, 131073, seed);
            }
    const long splitCases = g_cases - blockCases;
    if (argc > 1) run_huf_streams(argv[1]);
    const long hufCases = g_cases - blockCases - splitCases;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("blocks: %ld split: %ld huff0 streams: %ld threads: %u\n", blockCases, splitCases, hufCases, nThreads);
    printf("cases: %ld mismatches: %ld seconds: %.1f\n", (long)g_cases, (long)g_bad, secs);
    return g_bad ? 1 : 0;
}
