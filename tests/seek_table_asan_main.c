/* tests/seek_table_asan_main.c — TEST INFRASTRUCTURE ONLY: the seek table codec (lizard_amd/csrc/lizard_seek_host.c) as a stand-alone
 * program, built by tests/test_seek_table.py with -fsanitize=address,undefined.  Every buffer is a heap allocation of EXACTLY the
 * bytes the codec may touch, so a read in front of the tail, or a write behind the capacity, stops the program.  Round trips for
 * n = 1, 2, 1000; every tail length of a 3-item table (the codec must ask for more, and never read what it was not given); every
 * single-byte change of the table frame (never a crash, and USABLE only with entries that obey the rules). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/lizard_amd.h"

#define CHECK(c) do { if (!(c)) { printf("seek_table_asan_main: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int obeys(const LizardGPU_seekEntry_t* e, size_t n, uint64_t tableOffset)
{
    size_t i;
    if (!n || e[0].offset) return 0;
    for (i = 0; i < n; i++) {
        const uint64_t next = i + 1 < n ? e[i + 1].offset : tableOffset;
        if (e[i].flags || next > tableOffset || e[i].offset + e[i].prefixBytes >= next) return 0;
    }
    return 1;
}

static int round_trip(size_t n)
{
    const size_t bytes = LizardGPU_seekTableBytes(n);
    LizardGPU_seekEntry_t *in = (LizardGPU_seekEntry_t*)malloc(n * sizeof *in), *out = (LizardGPU_seekEntry_t*)malloc(n * sizeof *out);
    uint8_t *exact, *shorter, *tail;
    uint64_t pos = 0, at = 0;
    size_t i, got = 0, k;
    CHECK(in && out && bytes == 24 * n + 24);
    for (i = 0; i < n; i++) {
        in[i].offset = pos; in[i].prefixBytes = (uint32_t)(i % 3 ? 56 + 8 * (i % 5) : 0); in[i].decodedBytes = i * 1000003ull; in[i].flags = 0;
        pos += in[i].prefixBytes + 19 + i % 7;
    }
    exact = (uint8_t*)malloc(bytes);
    shorter = (uint8_t*)malloc(bytes - 1);
    CHECK(exact && shorter);
    CHECK(LizardGPU_seekTableWrite(shorter, bytes - 1, in, n) == 0);             /* no room: nothing, and nothing written behind */
    CHECK(LizardGPU_seekTableWrite(exact, bytes, in, n) == bytes);
    CHECK(LizardGPU_seekTableWrite(exact, bytes, in, 0) == 0 && LizardGPU_seekTableWrite(NULL, bytes, in, n) == 0);
    CHECK(LizardGPU_seekTableRead(exact, bytes, pos + bytes, out, n, &got, &at) == LIZARDGPU_SEEK_USABLE);
    CHECK(got == n && at == pos && !memcmp(in, out, n * sizeof *in) && obeys(out, n, at));
    /* the footer alone asks for the table; every tail in between too; each tail is its own allocation */
    for (k = 0; k < bytes; k += (n > 3 && k > 40 && k + 40 < bytes) ? 997 : 1) {
        tail = (uint8_t*)malloc(k ? k : 1);
        CHECK(tail);
        memcpy(tail, exact + bytes - k, k);
        got = 12345;
        CHECK(LizardGPU_seekTableRead(tail, k, pos + bytes, NULL, 0, &got, &at) == LIZARDGPU_SEEK_MORE);
        CHECK(got == (k < 16 ? 0 : n) && LizardGPU_seekTableBytes(got) > k);
        free(tail);
    }
    /* a short entries array: the first ones, and the whole count */
    memset(out, 0xEE, n * sizeof *out);
    CHECK(LizardGPU_seekTableRead(exact, bytes, pos + bytes, out, n / 2, &got, &at) == LIZARDGPU_SEEK_USABLE && got == n);
    CHECK(!memcmp(in, out, (n / 2) * sizeof *in) && (n / 2 == n || ((uint8_t*)(out + n / 2))[0] == 0xEE));
    free(in); free(out); free(exact); free(shorter);
    return 0;
}

static int every_byte_changed(void)
{
    LizardGPU_seekEntry_t in[3] = { { 0, 70000, 56, 0 }, { 400, 0, 0, 0 }, { 419, 131073, 64, 0 } }, out[3];
    const size_t bytes = LizardGPU_seekTableBytes(3);
    const uint64_t total = 9000 + bytes;
    uint8_t* t = (uint8_t*)malloc(bytes);
    size_t i, got;
    uint64_t at;
    int bit, usable = 0;
    CHECK(t && LizardGPU_seekTableWrite(t, bytes, in, 3) == bytes);
    for (i = 0; i < bytes; i++)
        for (bit = 0; bit < 8; bit++) {
            int rc;
            t[i] ^= (uint8_t)(1 << bit);
            rc = LizardGPU_seekTableRead(t, bytes, total, out, 3, &got, &at);
            CHECK(rc == LIZARDGPU_SEEK_USABLE || rc == LIZARDGPU_SEEK_NONE || rc == LIZARDGPU_SEEK_DAMAGED || rc == LIZARDGPU_SEEK_MORE);
            if (rc == LIZARDGPU_SEEK_MORE) CHECK(i >= bytes - 16 && i < bytes - 8 && got > 3 && LizardGPU_seekTableBytes(got) <= total);   /* only a larger n that the stream could hold */
            if (rc == LIZARDGPU_SEEK_USABLE) { usable++; CHECK(got == 3 && at == 9000 && obeys(out, 3, at)); }
            if (i < 8 || i >= bytes - 16 || (i - 8) % 24 >= 20) CHECK(rc != LIZARDGPU_SEEK_USABLE);      /* header, footer, flags: every bit counts */
            t[i] ^= (uint8_t)(1 << bit);
        }
    CHECK(usable > 0);                                         /* (a decoded size, a low bit of an offset: still a table that obeys the rules) */
    CHECK(LizardGPU_seekTableRead(t, bytes, bytes - 1, out, 3, &got, &at) == -LIZARDGPU_ERR_ARG);
    CHECK(LizardGPU_seekTableRead(NULL, 0, total, out, 3, &got, &at) == -LIZARDGPU_ERR_ARG);
    CHECK(LizardGPU_seekTableRead(t + bytes - 40, 40, 40, out, 3, &got, &at) == LIZARDGPU_SEEK_NONE);     /* a stream too short for any table */
    free(t);
    return 0;
}

int main(void)
{
    CHECK(LizardGPU_seekTableBytes(0) == 24 && LizardGPU_seekTableBytes(1) == 48);
    CHECK(LizardGPU_seekTableBytes(178956969u) == 24ull * 178956969u + 24);       /* 24 n + 16 = 2^32 - 24: the last that fits */
    CHECK(LizardGPU_seekTableBytes(178956970u) == (size_t)-(long)LIZARDGPU_FRAME_ERR_GENERIC);
    if (round_trip(1) || round_trip(2) || round_trip(3) || round_trip(1000) || every_byte_changed()) return 1;
    printf("seek_table_asan_main: ok\n");
    return 0;
}
