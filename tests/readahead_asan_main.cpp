// tests/readahead_asan_main.cpp — TEST INFRASTRUCTURE ONLY: the source read-ahead of the level-10 producers (lizard_amd/csrc/lz_touch.h)
// on the CPU, as a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_source_readahead_emul.py builds
// and runs it; nothing is loaded into python).  The host form of a touch is a real read of the touched bytes, the source of a case is malloc(n) with
// the block at its start, and the ragged batch is one malloc whose last block ends at its last byte and whose blocks start at odd
// addresses: a touch before a source, behind it, or in the redzone between two allocations ends the program with a report.  The
// kernel's own areas are exact as well (tests/emul/readahead_api.cpp).  Every output is compared with the oracle's.
//
// Sizes: 21, 22, 1 023, 1 024, 1 025, 4 096, 131 072, 131 072 + 13, 131 072 + 9 000, 262 144, each as P50 data and as noise; one block
// of 131 072 + 9 000 bytes that repeats 515 bytes; the ragged batch over two producers and over one.
// Last line: "cases: N mismatches: M touches: T"; exit status 0 only with M == 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../oracle/lizard_oracle.h"

extern "C" long emul_readahead_split(const void* src, int nBlocks, const unsigned long long* srcOffsets, const unsigned* srcSizes, void* dst,
                                     int dstStride, unsigned* sizes, int level, int nProd, int nCons, unsigned seed, unsigned long long* log, long logCap);

namespace {
long g_cases = 0, g_bad = 0, g_touches = 0;
uint32_t rng_next(uint32_t& s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }

// blocks[i] = (offset, size) inside `area` (exactly areaBytes, a heap allocation of its own)
void run_batch(const char* what, const uint8_t* area, const std::vector<std::pair<size_t, unsigned>>& blocks, int nProd, unsigned seed)
{
    const int nb = (int)blocks.size();
    unsigned maxN = 0;
    std::vector<unsigned long long> offs; std::vector<unsigned> ns;
    for (const auto& b : blocks) { offs.push_back(b.first); ns.push_back(b.second); if (b.second > maxN) maxN = b.second; }
    const int stride = lzo_compress_bound((int)maxN);
    uint8_t* const dst = (uint8_t*)malloc((size_t)nb * (size_t)stride);
    uint8_t* const want = (uint8_t*)malloc((size_t)stride);
    unsigned* const sizes = (unsigned*)malloc(4u * (size_t)nb);
    memset(dst, 0xC3, (size_t)nb * (size_t)stride);
    for (int b = 0; b < nb; b++) sizes[b] = 0xA5A5A5A5u;
    const long cap = 1 << 16;
    unsigned long long* const log = (unsigned long long*)malloc(16u * (size_t)cap);
    const long events = emul_readahead_split(area, nb, offs.data(), ns.data(), dst, stride, sizes, 10, nProd, 1, seed, log, cap);
    g_cases++;
    if (events < 0) { g_bad++; fprintf(stderr, "MISMATCH %s: refused\n", what); }
    for (long i = 0; i < events && i < cap; i++) if (!(log[2 * i + 1] >> 32)) g_touches++;
    for (int b = 0; events >= 0 && b < nb; b++) {
        const int w = lzo_compress(area + blocks[(size_t)b].first, want, (int)ns[(size_t)b], stride, 10);
        if (w <= 0 || sizes[b] != (unsigned)w || memcmp(dst + (size_t)b * (size_t)stride, want, (size_t)w)) {
            g_bad++;
            fprintf(stderr, "MISMATCH %s block %d (%u bytes): size %u, oracle %d\n", what, b, ns[(size_t)b], sizes[b], w);
        }
    }
    free(dst); free(want); free(sizes); free(log);
}

void run_one(const char* kind, unsigned n, unsigned seed)
{
    uint8_t* const src = (uint8_t*)malloc(n);                               // exactly n: a touch behind the block is a report
    if (!strcmp(kind, "p50")) lzo_datagen(src, n, 0.5, 0.0, 40u + n % 97u);
    else if (!strcmp(kind, "noise")) { uint32_t s = 0x9E3779B9u ^ n; for (unsigned i = 0; i < n; i++) src[i] = (uint8_t)(rng_next(s) >> 11); }
    else { uint32_t s = 515u; uint8_t period[515]; for (int i = 0; i < 515; i++) period[i] = (uint8_t)(rng_next(s) >> 11); for (unsigned i = 0; i < n; i++) src[i] = period[i % 515u]; }
    char what[64]; snprintf(what, sizeof what, "%s %u", kind, n);
    run_batch(what, src, { { 0, n } }, 1, seed);
    free(src);
}
}  // namespace

int main()
{
    const unsigned sizes[] = { 21, 22, 1023, 1024, 1025, 4096, 131072, 131072 + 13, 131072 + 9000, 262144 };
    unsigned seed = 1;
    for (unsigned n : sizes) { run_one("p50", n, seed++); run_one("noise", n, seed++); }
    run_one("repeat515", 131072 + 9000, seed++);
    // the ragged batch of tests/source_readahead_inputs.py: (bytes in front, size); odd starts, the last block ends the allocation
    const unsigned ragged[][2] = { { 1, 1025 }, { 1, 4109 }, { 3, 21 }, { 1, 131072 + 13 }, { 1, 9001 } };
    size_t total = 0;
    std::vector<std::pair<size_t, unsigned>> blocks;
    for (const auto& r : ragged) { total += r[0]; blocks.push_back({ total, r[1] }); total += r[1]; }
    uint8_t* const area = (uint8_t*)malloc(total);
    lzo_datagen(area, total, 0.5, 0.0, 77u);
    run_batch("ragged, two producers", area, blocks, 2, seed++);
    run_batch("ragged, one producer", area, blocks, 1, seed++);
    free(area);
    printf("cases: %ld mismatches: %ld touches: %ld\n", g_cases, g_bad, g_touches);
    return g_bad ? 1 : 0;
}
