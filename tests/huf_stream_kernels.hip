// tests/huf_stream_kernels.hip — TEST INFRASTRUCTURE: lz_put_stream_huf (lizard_amd/csrc/lz_huf.h), the huff0 stage of levels >= 30,
// on its own on the device, stream by stream.  The product reaches the stage only through whole blocks, where the parse decides what
// the flag and literal streams look like; here every stream of tests/huf_stream_inputs.py — built for one path of the stage each: RLE,
// "not compressible", the depth limiter's two repayment loops, trees of 64 .. 256 leaves, both weight headers, FSE_normalizeM2, the
// packer's partial lane group, sizes around every step — goes through the product's own primitives (v_readlane / v_writelane tables,
// ds_bpermute, the DPP scans, ds_or into the LDS ring, unaligned dword stores) in three forms:
//   (a) one wave per workgroup, one stream per wave, the workspace 512 words of __shared__ memory filled with 0x77777777; the stream
//       starts 0, 1, 3 or 15 bytes behind a 16-byte boundary and the output 0, 1, 2 or 3 bytes behind a dword boundary;
//   (b) one wave per workgroup, 8 streams one after the other through the same workspace, nothing cleared in between;
//   (c) 4 workgroups of 8 waves that share a pool of 3 workspaces (LzHufPool, lz_pool_acquire / lz_pool_release, lz_block.h): a wave
//       claims the next pair of streams with lz_claim_index, acquires a workspace, writes the two streams one behind the other as
//       lz_write_subblock_seq does, and releases; the pool's mask word starts at 0.
// The expected bytes (the oracle's, computed by the Python side) come with the streams in the case file argv[1] (layout:
// tests/huf_stream_inputs.py, write_case_file); no oracle is linked.  A stream of n bytes may change only the n + 3 bytes at its
// output position; those behind the size it returns are unspecified; everything else — the gaps between the outputs, 64-byte canaries
// around every device buffer, the streams themselves — must be as it was.  Every HIP call is checked.
//   hipcc -O2 --offload-arch=gfx950 tests/huf_stream_kernels.hip -o tests/huf_stream_kernels
//   tests/huf_stream_kernels CASEFILE      prints "cases: N mismatches: 0" (N = 3 x streams), exit 0
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../lizard_amd/csrc/lz_block.h"

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "huf_stream_kernels: %s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

struct Job { const u8* src; u8* out; u32 n; u32 pad; };
struct Res { u32 size, huffed; };

constexpr u32 kPoolSlots = 3, kPoolWaves = 8, kPoolGroups = 4, kSeqLen = 8;
constexpr u32 kWsFill = 0x77777777u;

// (a): perBlock = 1; (b): workgroup g takes the streams g, g + stride, g + 2 stride, ... (neighbours in the set are alike; these are not)
__global__ __launch_bounds__(64) void huf_single_kernel(const Job* jobs, Res* res, u32 nJobs, u32 perBlock, u32 stride)
{
    __shared__ u32 ws[LZ_HUF_WS_WORDS];
    const u32 lane = lz_lane();
    for (u32 i = lane; i < LZ_HUF_WS_WORDS; i += 64u) ws[i] = kWsFill;
    lz_lds_sync();
    for (u32 k = 0; k < perBlock; k++) {
        lz_converge();
        const u32 j = blockIdx.x + k * stride;
        if (j >= nJobs) break;
        u32 h = 0;
        const u32 r = lz_put_stream_huf((u8*)lz_uniform64((u64)jobs[j].out), (const u8*)lz_uniform64((u64)jobs[j].src), lz_uniform(jobs[j].n), ws, &h);
        if (lane == 0) { res[j].size = r; res[j].huffed = h; }
        lz_converge();
    }
}

// (c): jobs[2p].out is where pair p starts; the second stream of a pair goes where the first one ended
__global__ __launch_bounds__(64 * kPoolWaves) void huf_pool_kernel(const Job* jobs, Res* res, u32 nJobs, u32* counter)
{
    __shared__ u32 poolMem[kPoolSlots][LZ_HUF_WS_WORDS];
    __shared__ u32 poolMask;
    for (u32 i = threadIdx.x; i < kPoolSlots * LZ_HUF_WS_WORDS; i += blockDim.x) (&poolMem[0][0])[i] = kWsFill;
    if (threadIdx.x == 0) poolMask = 0;
    __syncthreads();
    LzHufPool pool; pool.base = &poolMem[0][0]; pool.mask = &poolMask; pool.count = kPoolSlots; pool.stride = LZ_HUF_WS_WORDS;
    const u32 nPairs = (nJobs + 1u) / 2u;
    for (;;) {
        lz_converge();
        const u32 p = lz_claim_index(counter);
        if (p >= nPairs) break;
        const u32 j0 = 2u * p, j1 = j0 + 1u;
        u32 h0 = 0, h1 = 0, r1 = 0, slot;
        u8* q = (u8*)lz_uniform64((u64)jobs[j0].out);
        u32* const ws = lz_pool_acquire(pool, slot);
        const u32 r0 = lz_put_stream_huf(q, (const u8*)lz_uniform64((u64)jobs[j0].src), lz_uniform(jobs[j0].n), ws, &h0);
        q += r0;
        if (j1 < nJobs) r1 = lz_put_stream_huf(q, (const u8*)lz_uniform64((u64)jobs[j1].src), lz_uniform(jobs[j1].n), ws, &h1);
        lz_pool_release(pool, slot);
        if (lz_lane() == 0) {
            res[j0].size = r0; res[j0].huffed = h0;
            if (j1 < nJobs) { res[j1].size = r1; res[j1].huffed = h1; }
        }
        lz_converge();
    }
}

namespace {
const size_t kGuard = 64, kGap = 64;
const uint8_t kCanary = 0xC3;
int g_cases, g_bad;

void mismatch(const char* form, const std::string& name, const char* what, size_t at, uint64_t got, uint64_t want)
{
    if (g_bad++ < 30) fprintf(stderr, "huf_stream_kernels: %s %s: %s: at %zu got %llu, want %llu\n", form, name.c_str(), what, at, (unsigned long long)got, (unsigned long long)want);
}

struct Dev {
    uint8_t* base = nullptr; size_t n = 0;
    explicit Dev(size_t bytes) : n(bytes) { CK(hipMalloc((void**)&base, n + 2 * kGuard)); CK(hipMemset(base, kCanary, n + 2 * kGuard)); }
    Dev(const Dev&) = delete;
    ~Dev() { CK(hipFree(base)); }
    uint8_t* p() const { return base + kGuard; }                 // (hipMalloc aligns to 256 bytes and kGuard is 64: p() is 16-byte aligned)
    void put(const void* h) { if (n) CK(hipMemcpy(p(), h, n, hipMemcpyHostToDevice)); }
    std::vector<uint8_t> get(const char* form, const char* what) const
    {
        std::vector<uint8_t> h(n + 2 * kGuard);
        CK(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kGuard; i++) {
            if (h[i] != kCanary) mismatch(form, what, "canary in front", i, h[i], kCanary);
            if (h[kGuard + n + i] != kCanary) mismatch(form, what, "canary behind", i, h[kGuard + n + i], kCanary);
        }
        return std::vector<uint8_t>(h.begin() + kGuard, h.begin() + kGuard + n);
    }
};

struct Case { std::string name; std::vector<uint8_t> data, want; uint32_t huffed; };

std::vector<Case> load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "huf_stream_kernels: cannot open %s\n", path); exit(2); }
    auto need = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "huf_stream_kernels: %s is truncated\n", path); exit(2); } };
    char magic[4]; uint32_t count;
    need(magic, 4); need(&count, 4);
    if (memcmp(magic, "HUFS", 4) || count == 0 || count > 100000u) { fprintf(stderr, "huf_stream_kernels: %s is not a case file\n", path); exit(2); }
    std::vector<Case> cases(count);
    for (Case& c : cases) {
        uint32_t h[4];                                             // name length, n, size of the expected bytes, huffed
        need(h, sizeof h);
        if (h[0] > 256u || h[1] == 0 || h[1] > 131072u || h[2] > h[1] + 3u || h[3] > 1u) { fprintf(stderr, "huf_stream_kernels: bad record in %s\n", path); exit(2); }
        c.name.resize(h[0]); c.data.resize(h[1]); c.want.resize(h[2]); c.huffed = h[3];
        need(&c.name[0], h[0]); need(c.data.data(), h[1]); need(c.want.data(), h[2]);
    }
    fclose(f);
    return cases;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
const size_t kSrcOff[4] = { 0, 1, 3, 15 }, kOutOff[4] = { 0, 1, 2, 3 };

// The streams in one device buffer for all three forms: stream i starts kSrcOff[i % 4] bytes behind a 16-byte boundary.
struct Sources {
    std::vector<size_t> at; std::vector<uint8_t> host;
    explicit Sources(const std::vector<Case>& cases)
    {
        size_t cur = 0;
        for (size_t i = 0; i < cases.size(); i++) { at.push_back(align_up(cur, 16) + kSrcOff[i % 4]); cur = at.back() + cases[i].data.size() + kGap; }
        host.assign(cur, 0x5A);
        for (size_t i = 0; i < cases.size(); i++) memcpy(&host[at[i]], cases[i].data.data(), cases[i].data.size());
    }
};

// One form: lay the outputs out, run, compare.  paired: the streams 2p, 2p + 1 share one output area, the second behind the first.
void run_form(const char* form, const std::vector<Case>& cases, const Sources& S, const Dev& dSrc, bool paired, uint32_t perBlock)
{
    const uint32_t N = (uint32_t)cases.size();
    std::vector<size_t> at(N), len(N);                             // output area of stream i (paired: of the pair, at the even one)
    size_t cur = 0;
    for (uint32_t i = 0; i < N; i++) {
        if (paired && (i & 1u)) { at[i] = at[i - 1]; len[i] = len[i - 1]; continue; }
        len[i] = cases[i].data.size() + 3 + (paired && i + 1 < N ? cases[i + 1].data.size() + 3 : 0);
        const uint32_t rot = paired ? i / 2 : i / 4;               // with the source's i % 4: all sixteen pairs of residues
        at[i] = align_up(cur, 4) + kOutOff[rot % 4];
        cur = at[i] + len[i] + kGap;
    }
    Dev dOut(cur), dJobs(N * sizeof(Job)), dRes(N * sizeof(Res)), dCounter(4);
    std::vector<Job> jobs(N);
    for (uint32_t i = 0; i < N; i++) { jobs[i].src = dSrc.p() + S.at[i]; jobs[i].out = dOut.p() + at[i]; jobs[i].n = (u32)cases[i].data.size(); jobs[i].pad = 0; }
    dJobs.put(jobs.data());
    const uint32_t zero = 0; dCounter.put(&zero);
    if (paired) hipLaunchKernelGGL(huf_pool_kernel, dim3(kPoolGroups), dim3(64 * kPoolWaves), 0, 0, (const Job*)dJobs.p(), (Res*)dRes.p(), N, (u32*)dCounter.p());
    else {
        const uint32_t groups = (N + perBlock - 1) / perBlock;
        hipLaunchKernelGGL(huf_single_kernel, dim3(groups), dim3(64), 0, 0, (const Job*)dJobs.p(), (Res*)dRes.p(), N, perBlock, groups);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    const std::vector<uint8_t> out = dOut.get(form, "output buffer"), r = dRes.get(form, "results");
    const Res* res = (const Res*)r.data();
    std::vector<uint8_t> may(out.size(), 0);                       // 1: a byte the stage may have written
    for (uint32_t i = 0; i < N; i++) {
        const Case& c = cases[i];
        size_t start = at[i];
        if (paired && (i & 1u)) start += res[i - 1].size <= cases[i - 1].data.size() + 3 ? res[i - 1].size : 0;
        const bool same = res[i].size == c.want.size() && res[i].huffed == c.huffed;
        if (res[i].size != c.want.size()) mismatch(form, c.name, "size", 0, res[i].size, c.want.size());
        if (res[i].huffed != c.huffed) mismatch(form, c.name, "huffed", 0, res[i].huffed, c.huffed);
        if (same) {
            for (size_t k = 0; k < c.want.size(); k++)
                if (out[start + k] != c.want[k]) { mismatch(form, c.name, "bytes", k, out[start + k], c.want[k]); break; }
        }
        for (size_t k = 0; k < c.data.size() + 3 && start + k < at[i] + len[i]; k++) may[start + k] = 1;
        g_cases++;
    }
    for (size_t k = 0; k < out.size(); k++)
        if (!may[k] && out[k] != kCanary) { mismatch(form, "output buffer", "a byte outside every stream's n + 3 changed", k, out[k], kCanary); break; }
    if (dJobs.get(form, "job table") != std::vector<uint8_t>((uint8_t*)jobs.data(), (uint8_t*)(jobs.data() + N))) mismatch(form, "job table", "changed", 0, 1, 0);
    if (dSrc.get(form, "streams") != S.host) mismatch(form, "streams", "the source bytes changed", 0, 1, 0);
    if (paired) {
        const std::vector<uint8_t> c = dCounter.get(form, "counter");
        uint32_t v; memcpy(&v, c.data(), 4);
        const uint32_t want = (N + 1) / 2 + kPoolGroups * kPoolWaves;  // every pair once, and one claim past the end per wave
        if (v != want) mismatch(form, "counter", "claims", 0, v, want);
    }
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: huf_stream_kernels CASEFILE\n"); return 2; }
    const std::vector<Case> cases = load(argv[1]);
    const Sources S(cases);
    Dev dSrc(S.host.size());
    dSrc.put(S.host.data());
    run_form("(a) one stream per wave", cases, S, dSrc, false, 1);
    run_form("(b) eight streams through one workspace", cases, S, dSrc, false, kSeqLen);
    run_form("(c) pairs through a pool of three workspaces", cases, S, dSrc, true, 0);
    printf("cases: %d mismatches: %d\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
