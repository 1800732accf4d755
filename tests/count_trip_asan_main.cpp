// tests/count_trip_asan_main.cpp — TEST INFRASTRUCTURE ONLY: the count trips behind a winner of the level-10 producers' round
// (lizard_amd/csrc/lz_block.h: the late back trip) on the CPU, as a program of its own under AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_count_trip_emul.py builds and runs it; nothing is loaded into python).  argv[1] names a file of
// blocks (u32 count, then per block u32 size and the bytes: the inputs of tests/count_trip_inputs.py).  The source of a case is
// malloc(n) with the block at its start, so a read in front of a block or behind it ends the program with a report; the kernel's own
// areas are exact as well (tests/emul/count_trip_api.cpp).  Every block runs at levels 10 and 30 and is compared with the oracle's.
// Last line: "cases: N mismatches: M late: L" (the mark of the late back trips); exit status 0 only with M == 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../oracle/lizard_oracle.h"

extern "C" int emul_ct_split(const void* src, int nBlocks, const unsigned long long* srcOffsets, const unsigned* srcSizes, void* dst,
                             int dstStride, unsigned* sizes, int level, int nProd, int nCons, int laneForms, unsigned seed);
extern "C" void emul_ct_marks(unsigned long long out[16], int reset);

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: count_trip_asan_main blocks.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    long cases = 0, bad = 0;
    for (uint32_t b = 0; b < count; b++) {
        uint32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n == 0) return 2;
        uint8_t* const src = (uint8_t*)malloc(n);                            // exactly n
        if (fread(src, 1, n, f) != n) return 2;
        const int stride = lzo_compress_bound((int)n);
        uint8_t* const dst = (uint8_t*)malloc((size_t)stride);
        uint8_t* const want = (uint8_t*)malloc((size_t)stride);
        const int levels[2] = { 10, 30 };
        for (int level : levels) {
            const unsigned long long off = 0;
            unsigned size = 0xA5A5A5A5u;
            memset(dst, 0xC3, (size_t)stride);
            const int rc = emul_ct_split(src, 1, &off, &n, dst, stride, &size, level, 1, 1, -1, b + 1u);
            const int w = lzo_compress(src, want, (int)n, stride, level);
            cases++;
            if (rc != 0 || w <= 0 || size != (unsigned)w || memcmp(dst, want, (size_t)w)) {
                bad++;
                fprintf(stderr, "MISMATCH block %u (%u bytes) level %d: size %u, oracle %d\n", b, n, level, size, w);
            }
        }
        free(src); free(dst); free(want);
    }
    fclose(f);
    unsigned long long marks[16];
    emul_ct_marks(marks, 0);
    printf("cases: %ld mismatches: %ld late: %llu\n", cases, bad, marks[3]);
    return bad ? 1 : 0;
}
