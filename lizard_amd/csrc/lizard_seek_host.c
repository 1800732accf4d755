/* lizard_seek_host.c — the seek table of a seekable stream (include/lizard_amd.h Part 3b): the skippable frame at the end of a stream
 * that says where every item starts.  Plain C, no HIP, no allocation: LizardGPU_seekTableBytes / Write / Read work on host bytes alone
 * and are what the device entries (lizard_seek_device.c) and the table kernel's tests are judged against.  Every field is read and
 * written byte by byte, little-endian, at any address. */
#include <stddef.h>
#include <stdint.h>

#include "../../include/lizard_amd.h"

#define SK_ENTRY   24u
#define SK_FOOTER  16u
#define SK_HEADER  8u
#define SK_MAX_N   ((0xFFFFFFFFull - SK_FOOTER) / SK_ENTRY)      /* the largest n whose 24 n + 16 fits the u32 size field */

static void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static void put64(uint8_t* p, uint64_t v) { put32(p, (uint32_t)v); put32(p + 4, (uint32_t)(v >> 32)); }
static uint32_t get32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint64_t get64(const uint8_t* p) { return (uint64_t)get32(p) | ((uint64_t)get32(p + 4) << 32); }

/* 24 n + 24, or 0 when the size field (or a size_t) cannot hold it */
static size_t sk_bytes(size_t n)
{
    if ((uint64_t)n > SK_MAX_N || (uint64_t)n * SK_ENTRY + SK_HEADER + SK_FOOTER > (uint64_t)(size_t)-1 / 2) return 0;
    return n * SK_ENTRY + SK_HEADER + SK_FOOTER;
}

size_t LizardGPU_seekTableBytes(size_t n)
{
    const size_t bytes = sk_bytes(n);
    return bytes ? bytes : (size_t)-(long)LIZARDGPU_FRAME_ERR_GENERIC;
}

size_t LizardGPU_seekTableWrite(void* dst, size_t dstCapacity, const LizardGPU_seekEntry_t* entries, size_t n)
{
    const size_t bytes = sk_bytes(n);
    uint8_t* p = (uint8_t*)dst;
    size_t i;
    if (!dst || !entries || !n || !bytes || bytes > dstCapacity) return 0;
    put32(p, LIZARDGPU_SEEK_MAGIC);
    put32(p + 4, (uint32_t)(bytes - SK_HEADER));
    p += SK_HEADER;
    for (i = 0; i < n; i++, p += SK_ENTRY) {
        put64(p, entries[i].offset);
        put64(p + 8, entries[i].decodedBytes);
        put32(p + 16, entries[i].prefixBytes);
        put32(p + 20, entries[i].flags);
    }
    put64(p, (uint64_t)n);
    put32(p + 8, LIZARDGPU_SEEK_VERSION);
    put32(p + 12, LIZARDGPU_SEEK_TAG);
    return bytes;
}

int LizardGPU_seekTableRead(const void* tail, size_t tailBytes, uint64_t streamBytes, LizardGPU_seekEntry_t* entries, size_t maxEntries,
                            size_t* nPtr, uint64_t* tableOffsetPtr)
{
    const uint8_t* const t = (const uint8_t*)tail;
    const uint8_t *foot, *head, *p;
    uint64_t n, need, tableOffset, sum = 0, i;
    if (!tail || !nPtr || !tableOffsetPtr || (uint64_t)tailBytes > streamBytes) return -LIZARDGPU_ERR_ARG;
    *nPtr = 0;
    *tableOffsetPtr = 0;
    if (streamBytes < SK_HEADER + SK_ENTRY + SK_FOOTER) return LIZARDGPU_SEEK_NONE;
    if (tailBytes < SK_FOOTER) return LIZARDGPU_SEEK_MORE;
    foot = t + tailBytes - SK_FOOTER;
    if (get32(foot + 12) != LIZARDGPU_SEEK_TAG) return LIZARDGPU_SEEK_NONE;
    if (get32(foot + 8) != LIZARDGPU_SEEK_VERSION) return LIZARDGPU_SEEK_DAMAGED;
    n = get64(foot);
    if (n < 1 || n > SK_MAX_N) return LIZARDGPU_SEEK_DAMAGED;
    need = n * SK_ENTRY + SK_HEADER + SK_FOOTER;
    if (need > streamBytes) return LIZARDGPU_SEEK_DAMAGED;
    *nPtr = (size_t)n;
    if ((uint64_t)tailBytes < need) return LIZARDGPU_SEEK_MORE;
    head = t + (tailBytes - (size_t)need);
    if (get32(head) != LIZARDGPU_SEEK_MAGIC || get32(head + 4) != (uint32_t)(need - SK_HEADER)) return LIZARDGPU_SEEK_DAMAGED;
    tableOffset = streamBytes - need;
    for (i = 0, p = head + SK_HEADER; i < n; i++, p += SK_ENTRY) {
        const uint64_t off = get64(p), dec = get64(p + 8), next = i + 1 < n ? get64(p + SK_ENTRY) : tableOffset;
        const uint32_t pre = get32(p + 16), flags = get32(p + 20);
        if (flags || (i == 0 && off != 0)) return LIZARDGPU_SEEK_DAMAGED;
        if (next > tableOffset || off >= next || (uint64_t)pre >= next - off) return LIZARDGPU_SEEK_DAMAGED;      /* off + pre < next <= tableOffset */
        if (sum + dec < sum) return LIZARDGPU_SEEK_DAMAGED;
        sum += dec;
        if (entries && i < (uint64_t)maxEntries) {
            entries[i].offset = off; entries[i].decodedBytes = dec; entries[i].prefixBytes = pre; entries[i].flags = 0;
        }
    }
    *tableOffsetPtr = tableOffset;
    return LIZARDGPU_SEEK_USABLE;
}
