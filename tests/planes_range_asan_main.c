/* tests/planes_range_asan_main.c — TEST INFRASTRUCTURE: lizard_amd/csrc/lizard_slice_host.c (LizardGPU_planesRangeBytes,
 * LizardGPU_frameRangesBound) as a stand-alone program for the sanitizer build (tests/test_planes_range.py).  Every array is a heap
 * allocation of exactly the entries the functions may touch, so that a write or a read one entry too far is a report.  The ranges
 * are checked against the layout's own formula, element by element: every byte an element of the range has a bit in lies in its
 * piece's range, the ranges ascend, and the bound is the sum of the covering blocks. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/lizard_amd.h"

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "planes_range_asan_main: line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 1; } } while (0)

static int one(uint64_t n, uint32_t E, uint32_t filter, uint64_t first, uint64_t last)
{
    const size_t pieces = filter ? 8 * (size_t)E + 1 : E;
    const uint64_t n8 = n - n % 8, P = n8 / 8;
    LizardGPU_byteRange_t* r = (LizardGPU_byteRange_t*)malloc(pieces * sizeof *r);
    LizardGPU_byteRange_t* tooSmall = (LizardGPU_byteRange_t*)malloc((pieces - 1) * sizeof *r + 1);
    uint64_t i, prev = 0;
    size_t q, got;
    CHECK(r && tooSmall, "allocation");
    CHECK(LizardGPU_planesRangeBytes(n, E, filter, first, last, tooSmall, pieces - 1) == 0, "room for one range too few was accepted");
    got = LizardGPU_planesRangeBytes(n, E, filter, first, last, r, pieces);
    CHECK(got == pieces, "%zu ranges, wanted %zu", got, pieces);
    for (q = 0; q < pieces; q++) {
        CHECK(r[q].lo <= r[q].hi && r[q].lo >= prev && r[q].hi <= n * E, "range %zu = [%llu, %llu) of n %llu E %u filter %u [%llu, %llu)", q,
              (unsigned long long)r[q].lo, (unsigned long long)r[q].hi, (unsigned long long)n, E, filter, (unsigned long long)first, (unsigned long long)last);
        prev = r[q].hi;
    }
    for (i = first; i < last; i++) {
        uint32_t k;
        for (k = 0; k < 8 * E; k++) {                          /* bit k of element i */
            uint64_t at;
            if (!filter) { q = k / 8; at = (k / 8) * n + i; }
            else if (i < n8) { q = k; at = k * P + i / 8; }
            else { q = 8 * E; at = i * E + k / 8; }
            CHECK(at >= r[q].lo && at < r[q].hi, "bit %u of element %llu lies at %llu, outside piece %zu", k, (unsigned long long)i, (unsigned long long)at, q);
        }
    }
    if (first == last) for (q = 0; q < pieces; q++) CHECK(r[q].lo == r[q].hi, "an empty element range with a non-empty byte range");
    {
        const size_t B = 64;
        size_t want = 0;
        for (q = 0; q < pieces; q++) if (r[q].hi > r[q].lo) want += (size_t)(((r[q].hi + B - 1) / B - r[q].lo / B) * B);
        CHECK(LizardGPU_frameRangesBound(r, pieces, B) == want, "the bound");
    }
    free(r); free(tooSmall);
    return 0;
}

int main(void)
{
    static const uint64_t sizes[] = { 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129 };
    static const uint32_t elems[] = { 1, 2, 4, 8 };
    size_t s, e;
    uint32_t filter;
    unsigned long long calls = 0;
    for (s = 0; s < sizeof sizes / sizeof sizes[0]; s++)
        for (e = 0; e < 4; e++)
            for (filter = 0; filter < 2; filter++) {
                uint64_t first, last;
                for (first = 0; first <= sizes[s]; first++)
                    for (last = first; last <= sizes[s]; last += (sizes[s] > 64 ? 3 : 1), calls++)
                        if (one(sizes[s], elems[e], filter, first, last)) return 1;
                if (one(sizes[s], elems[e], filter, 0, sizes[s])) return 1;
            }
    {
        LizardGPU_byteRange_t x = { 0, 1 };
        CHECK(LizardGPU_frameRangesBound(NULL, 0, 64) == 0 && LizardGPU_frameRangesBound(&x, 1, 0) == 0 && LizardGPU_frameRangesBound(&x, 0, 64) == 0, "the bound's refusals");
        CHECK(LizardGPU_planesRangeBytes(8, 3, 0, 0, 1, &x, 1) == 0 && LizardGPU_planesRangeBytes(8, 1, 2, 0, 1, &x, 1) == 0
              && LizardGPU_planesRangeBytes(8, 1, 0, 2, 1, &x, 1) == 0 && LizardGPU_planesRangeBytes(8, 1, 0, 0, 9, &x, 1) == 0, "refusals");
    }
    printf("planes_range_asan_main: ok, %llu calls\n", calls);
    return 0;
}
