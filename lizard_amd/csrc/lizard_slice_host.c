/* lizard_slice_host.c — the arithmetic of a row range of a tensor stream (include/lizard_amd.h Part 3d): which bytes of the SPLIT
 * content elements [first, last) of a buffer need (LizardGPU_planesRangeBytes), and how much room the blocks that cover byte ranges
 * take (LizardGPU_frameRangesBound).  Plain C, no HIP, no allocation: tests compile this file alone.
 *
 * The layouts are those of planes_kernels.h and bitplanes_kernels.h.  n elements of E bytes:
 *   byte planes   byte p of element i lies at p * n + i: one range per plane, [p * n + first, p * n + last).  E = 1 is one range.
 *   bit planes    n8 = n - n % 8 elements are transposed, P = n8 / 8 bytes per plane; bit k of element i lies in byte k * P + i / 8:
 *                 one range per plane, [k * P + first / 8, k * P + ceil(min(last, n8) / 8)), empty for first >= n8; and one more
 *                 behind them, over the elements of [first, last) at and behind n8, which lie raw at n8 * E: the last n % 8.
 * Every range holds exactly the bytes some element of [first, last) has a bit in; an empty element range gives empty byte ranges. */
#include <stddef.h>
#include <stdint.h>

#include "../../include/lizard_amd.h"

size_t LizardGPU_planesRangeBytes(uint64_t nElems, uint32_t elemSize, uint32_t filter, uint64_t first, uint64_t last,
                                  LizardGPU_byteRange_t* out, size_t maxOut)
{
    const uint64_t E = elemSize;
    size_t n = 0;
    if (!out || (E != 1 && E != 2 && E != 4 && E != 8) || first > last || last > nElems || nElems > (~(uint64_t)0) / 8) return 0;
    if (filter == LIZARDGPU_FILTER_BYTE_PLANES) {
        uint64_t p;
        if (maxOut < E) return 0;
        for (p = 0; p < E; p++, n++) { out[n].lo = p * nElems + first; out[n].hi = p * nElems + last; }
        return n;
    }
    if (filter == LIZARDGPU_FILTER_BIT_PLANES) {
        const uint64_t n8 = nElems - nElems % 8, P = n8 / 8;
        const uint64_t top = last < n8 ? last : n8;             /* the transposed elements of the range end here */
        const uint64_t lo = first < top ? first / 8 : P, hi = first < top ? (top + 7) / 8 : P;
        const uint64_t rawLo = first > n8 ? first : n8, rawHi = last > rawLo ? last : rawLo;
        uint64_t k;
        if (maxOut < 8 * E + 1) return 0;
        for (k = 0; k < 8 * E; k++, n++) { out[n].lo = k * P + lo; out[n].hi = k * P + hi; }
        out[n].lo = n8 * E + (rawLo - n8) * E; out[n].hi = n8 * E + (rawHi - n8) * E;
        return n + 1;
    }
    return 0;
}

size_t LizardGPU_frameRangesBound(const LizardGPU_byteRange_t* ranges, size_t nRanges, size_t blockSize)
{
    size_t i, total = 0;
    if (!ranges || !blockSize) return 0;
    for (i = 0; i < nRanges; i++) {
        const uint64_t lo = ranges[i].lo, hi = ranges[i].hi;
        if (hi <= lo) continue;                                  /* empty: no room */
        total += (size_t)(((hi - 1) / blockSize + 1 - lo / blockSize) * blockSize);
    }
    return total;
}
