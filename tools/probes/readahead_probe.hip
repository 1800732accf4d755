// readahead_probe.hip — bench tooling (not part of the library): what does it cost a wave to USE a source line for the first time, and
// does touching the line ahead of time help — through the scalar path (out of order, lgkmcnt) or the vector path (the wave's own
// in-order vmcnt queue)?  One wave per CU, then 13 waves per CU; every wave walks a 4 MiB region of its own, one line every 2 KiB, so
// that every line is a first touch that comes from HBM.  Clocks (s_memtime) from the issue of an 8-byte-per-lane vector load of ONE
// 128-byte line to its use:
//   cold        nobody has touched the line
//   l2hit       the same line again, past the vector L1 (sc1): the figure a successful read-ahead should give
//   scalar D    a scalar dword load of the line was issued D clocks earlier (its result is consumed behind the measured load's issue)
//   vector D    a vector load of the line was issued D clocks earlier and is still in the wave's queue, or has returned
//   scalar2 D   the same with a scalar dword load in EACH 64-byte half of the line
//   scalarH D   one scalar dword load, and the measured load confined to the 64-byte half it touched
//   scalarX D   ONE 8-byte scalar load across the middle of the line (bytes 60..67): the library's touch (lz_touch.h, LZ_RA_LINE 128)
//   behind-cold an L2-hit load (sc1, the previous line) issued directly behind a cold one and waited for: the in-order penalty itself
// "timer" is two clock reads back to back: what every figure above contains.  Per case the median over all waves of each wave's mean.
//   hipcc -O3 --offload-arch=gfx950 readahead_probe.hip -o readahead_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr uint32_t kIters = 128, kStride = 2048, kSlice = kIters * kStride;      // 256 KiB per case
constexpr uint64_t kRegion = 4ull << 20;                                          // per wave: the 16 slices of 256 KiB
constexpr int kDelays = 4;                                                        // sleeps of 1, 2, 4, 8 x s_sleep 8 (about 512 clocks each)
enum { C_TIMER = 0, C_COLD, C_L2HIT, C_SCALAR, C_VECTOR = C_SCALAR + kDelays, C_BEHIND = C_VECTOR + kDelays, C_SCALAR2, C_SCALARH = C_SCALAR2 + 2, C_SCALARX = C_SCALARH + 2, C_COUNT = C_SCALARX + 2 };

__device__ __forceinline__ uint64_t now() { uint64_t t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory"); return t; }
__device__ __forceinline__ uint64_t vld(const uint8_t* p) { uint64_t v; asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory"); return v; }
__device__ __forceinline__ uint64_t vld_l2(const uint8_t* p) { uint64_t v; asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory"); return v; }
__device__ __forceinline__ void vwait(uint64_t& a) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(a) :: "memory"); }
__device__ __forceinline__ void vwait2(uint64_t& a, uint64_t& b) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b) :: "memory"); }
// a scalar dword load of a uniform address, and the 8-byte form that is only dword-aligned
__device__ __forceinline__ uint32_t touch_scalar(const uint8_t* p)
{
    return __builtin_nontemporal_load((const __attribute__((address_space(4))) uint32_t*)((uintptr_t)p & ~(uintptr_t)3));
}
__device__ __forceinline__ uint64_t touch_scalar8(const uint8_t* p)
{
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef u32x2 __attribute__((aligned(4))) u32x2_a4;
    const u32x2_a4 v = __builtin_nontemporal_load((const __attribute__((address_space(4))) u32x2_a4*)((uintptr_t)p & ~(uintptr_t)3));
    return (uint64_t)v.x | ((uint64_t)v.y << 32);                                 // (a register pair: no instruction reads the result)
}
template <int K> __device__ __forceinline__ void delay() { for (int j = 0; j < K; j++) __builtin_amdgcn_s_sleep(8); }

// SCALAR 0: vector touch; 1: one scalar dword at the start of the line; 2: one in each 64-byte half of the line; 3: 8 bytes at 60
template <int K, int SCALAR>
__device__ __forceinline__ void touched(const uint8_t* slice, uint32_t lo, uint64_t& lat, uint64_t& dly, uint64_t& acc)
{
    for (uint32_t i = 0; i < kIters; i++) {
        const uint8_t* p = slice + i * kStride;
        const uint64_t t0 = now();
        uint32_t ts = 0, ts2 = 0; uint64_t tv = 0, ts8 = 0;
        if (SCALAR == 3) ts8 = touch_scalar8(p + 60); else if (SCALAR) ts = touch_scalar(p); else tv = vld(p + lo);
        if (SCALAR == 2) ts2 = touch_scalar(p + 64);
        delay<K>();
        const uint64_t t1 = now();
        uint64_t v = vld(p + lo);
        if (SCALAR) { asm volatile("" :: "s"(ts), "s"(ts2), "s"(ts8)); vwait(v); } else vwait2(tv, v);
        const uint64_t t2 = now();
        dly += t1 - t0; lat += t2 - t1; acc ^= v ^ tv;
    }
}

__global__ __launch_bounds__(1024) void probe(const uint8_t* base, uint32_t lineOff, uint64_t* out)
{
    const uint32_t lane = threadIdx.x & 63u, lo = (lane & 15u) * 8u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const uint8_t* reg = base + (uint64_t)wave * kRegion + lineOff;
    uint64_t lat[C_COUNT], dly[C_COUNT], acc = 0;
    for (int c = 0; c < C_COUNT; c++) lat[c] = dly[c] = 0;
    for (uint32_t i = 0; i < kIters; i++) {                                       // slice 0: timer, cold, l2hit
        const uint8_t* p = reg + i * kStride;
        uint64_t t0 = now(), t1 = now();
        lat[C_TIMER] += t1 - t0;
        t0 = now(); uint64_t v = vld(p + lo); vwait(v); t1 = now();
        lat[C_COLD] += t1 - t0; acc ^= v;
        t0 = now(); v = vld_l2(p + lo); vwait(v); t1 = now();
        lat[C_L2HIT] += t1 - t0; acc ^= v;
    }
    touched<1, 1>(reg + 1u * kSlice, lo, lat[C_SCALAR + 0], dly[C_SCALAR + 0], acc);
    touched<2, 1>(reg + 2u * kSlice, lo, lat[C_SCALAR + 1], dly[C_SCALAR + 1], acc);
    touched<4, 1>(reg + 3u * kSlice, lo, lat[C_SCALAR + 2], dly[C_SCALAR + 2], acc);
    touched<8, 1>(reg + 4u * kSlice, lo, lat[C_SCALAR + 3], dly[C_SCALAR + 3], acc);
    touched<1, 0>(reg + 5u * kSlice, lo, lat[C_VECTOR + 0], dly[C_VECTOR + 0], acc);
    touched<2, 0>(reg + 6u * kSlice, lo, lat[C_VECTOR + 1], dly[C_VECTOR + 1], acc);
    touched<4, 0>(reg + 7u * kSlice, lo, lat[C_VECTOR + 2], dly[C_VECTOR + 2], acc);
    touched<8, 0>(reg + 8u * kSlice, lo, lat[C_VECTOR + 3], dly[C_VECTOR + 3], acc);
    // the scalar path fills half a line?  Both halves touched; and one touch with the use confined to the touched half
    touched<2, 2>(reg + 10u * kSlice, lo, lat[C_SCALAR2 + 0], dly[C_SCALAR2 + 0], acc);
    touched<4, 2>(reg + 11u * kSlice, lo, lat[C_SCALAR2 + 1], dly[C_SCALAR2 + 1], acc);
    touched<2, 1>(reg + 12u * kSlice, lo & 63u, lat[C_SCALARH + 0], dly[C_SCALARH + 0], acc);
    touched<4, 1>(reg + 13u * kSlice, lo & 63u, lat[C_SCALARH + 1], dly[C_SCALARH + 1], acc);
    touched<2, 3>(reg + 14u * kSlice, lo, lat[C_SCALARX + 0], dly[C_SCALARX + 0], acc);
    touched<4, 3>(reg + 15u * kSlice, lo, lat[C_SCALARX + 1], dly[C_SCALARX + 1], acc);
    {                                                                             // slice 9: an L2 hit behind a cold load
        const uint8_t* s = reg + 9u * kSlice;
        uint64_t v = vld(s + lo); vwait(v); acc ^= v;
        for (uint32_t i = 1; i < kIters; i++) {
            const uint8_t* p = s + i * kStride;
            const uint64_t t0 = now();
            uint64_t a = vld(p + lo), b = vld_l2(p - kStride + lo);
            vwait2(a, b);
            const uint64_t t1 = now();
            lat[C_BEHIND] += (t1 - t0) * kIters / (kIters - 1u); acc ^= a ^ b;
        }
    }
    if (lane == 0) for (int c = 0; c < C_COUNT; c++) { out[((uint64_t)wave * C_COUNT + c) * 2u] = lat[c]; out[((uint64_t)wave * C_COUNT + c) * 2u + 1u] = dly[c]; }
    if (acc == 0x0123456789ABCDEFull) out[0] = acc;                               // (keeps the loads alive)
}

static double median(std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main()
{
    hipDeviceProp_t p; CK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount, maxWaves = 13;
    const size_t bytes = (size_t)cus * maxWaves * kRegion;
    uint8_t* base; uint64_t* out;
    CK(hipMalloc((void**)&base, bytes)); CK(hipMalloc((void**)&out, (size_t)cus * maxWaves * C_COUNT * 16));
    CK(hipMemset(base, 0x5A, bytes));
    std::vector<uint64_t> host((size_t)cus * maxWaves * C_COUNT * 2);
    static const char* const names[C_COUNT] = { "timer", "cold", "l2hit", "scalar D1", "scalar D2", "scalar D4", "scalar D8",
                                                "vector D1", "vector D2", "vector D4", "vector D8", "behind-cold",
                                                "scalar2 D2", "scalar2 D4", "scalarH D2", "scalarH D4", "scalarX D2", "scalarX D4" };
    int run = 0;
    for (int wpc : { 1, maxWaves }) {
        const int waves = cus * wpc;
        CK(hipMemset(out, 0, host.size() * 8));
        // (the second run reads other lines of the regions than the first: nothing it measures as cold was left in a cache)
        hipLaunchKernelGGL(probe, dim3(cus), dim3(64 * wpc), 0, 0, base, (uint32_t)(run++ * 1024), out);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(host.data(), out, host.size() * 8, hipMemcpyDeviceToHost));
        printf("%d wave%s per CU (%d waves, %u lines per case and wave): clocks, median over waves of the per-wave mean\n", wpc, wpc > 1 ? "s" : "", waves, kIters);
        for (int c = 0; c < C_COUNT; c++) {
            std::vector<double> l, d;
            for (int w = 0; w < waves; w++) { l.push_back((double)host[((size_t)w * C_COUNT + c) * 2] / kIters); d.push_back((double)host[((size_t)w * C_COUNT + c) * 2 + 1] / kIters); }
            const double ml = median(l), md = median(d);
            if (md > 0) printf("  %-12s issue-to-use %7.0f   (touched %5.0f clocks earlier; p10 %6.0f p90 %6.0f)\n", names[c], ml, md, l[l.size() / 10], l[l.size() * 9 / 10]);
            else        printf("  %-12s issue-to-use %7.0f   (p10 %6.0f p90 %6.0f)\n", names[c], ml, l[l.size() / 10], l[l.size() * 9 / 10]);
        }
    }
    return 0;
}
