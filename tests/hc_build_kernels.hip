// tests/hc_build_kernels.hip — TEST INFRASTRUCTURE: the chain build of the hashChain / noChain levels (lz_hc_begin, lz_hc_build,
// lz_hc_hits_plain / lz_hc_hits, lizard_amd/csrc/lz_hashchain.h) on its own on the device, table by table against the sequential
// model exported from the oracle (lzo_hc_tables, oracle/lizard_oracle.h, compiled into this program).  The product reaches these
// tables only through whole blocks, where the parse reads the few entries it happens to visit; here every entry of prev, chain2, hits
// and best of every input of tests/hc_build_inputs.py — built for one edge of the build each — is compared, after the build ran on
// the product's own primitives (the returning DS add / exchange whose lane order passes 1 and 2 rely on, the region pool of a
// workgroup), which the emulator of tests/test_hc_build_emul.py replaces.  A wave does what lz_compress_block does in front of the
// parse (lz_block.h, "if constexpr (PARSER == LZ_PARSER_HASHCHAIN)") and then copies its tables out.  Three forms:
//   (a) every job alone in a workgroup of one wave, a pool of LZ_HC_POOL + 1 regions;
//   (b) sixteen jobs in one workgroup of sixteen waves, large next to small, that queue for a pool of LZ_HC_POOL regions; several
//       workgroups at once;
//   (c) eight jobs in a row through ONE wave's slot, the largest first (the slot is laid out for it), nothing cleared in between.
// The two pool sizes are those of lz_wave_main (lz_kernels.h).  Every slot has exactly the size the library gives a wave
// (lizard_gpu.hip ensure_hc_slots: LZ_HC_SLOT_BYTES of the block size rounded up to 64 KiB, without best[] below levels 16 / 37), is
// filled with 0xB7 and lies between 64 canary bytes; the sources and the copied tables lie between canaries too.  Rules of the
// comparison: tests/test_hc_build_emul.py check_tables.  Every HIP call is checked.
//   hipcc -O2 --offload-arch=gfx950 tests/hc_build_kernels.hip oracle/lizard_oracle.c oracle/huf_oracle.c -o tests/hc_build_kernels
//   tests/hc_build_kernels CASEFILE      prints "cases: N mismatches: 0" (N = 3 x jobs), exit 0
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../lizard_amd/csrc/lz_block.h"
#include "../oracle/lizard_oracle.h"

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "hc_build_kernels: %s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

// lz_kernels.h (which declares every kernel of the library) has these two
#ifndef LZ_WAVES_HC
#define LZ_WAVES_HC 16
#endif
#ifndef LZ_HC_POOL
#define LZ_HC_POOL 3
#endif

struct Job { const u8* src; u8* slot; u8* out; u32 n, maxBlock, searchNum, pad; };

// out: hits words, prev, chain2, best (PRE) of the positions below nIns, each area rounded up to 8 bytes
__host__ __device__ inline size_t out_prev_at(u32 nIns) { return 8u * (((size_t)nIns + 63u) / 64u); }
__host__ __device__ inline size_t out_chain2_at(u32 nIns) { return out_prev_at(nIns) + ((2u * (size_t)nIns + 7u) & ~(size_t)7u); }
__host__ __device__ inline size_t out_best_at(u32 nIns) { return out_chain2_at(nIns) + ((4u * (size_t)nIns + 7u) & ~(size_t)7u); }
__host__ __device__ inline size_t out_bytes(u32 nIns, bool pre) { return out_best_at(nIns) + (pre ? ((4u * (size_t)nIns + 7u) & ~(size_t)7u) : 0u); }

// wave w of the grid runs the jobs waveFirst[w] .. waveFirst[w] + waveCount[w] - 1 one after the other
template <int SEARCHLEN, int HLOG, bool PRE, int NPOOL>
__global__ __launch_bounds__(64 * LZ_WAVES_HC) void hc_tables_kernel(const Job* jobs, const u32* waveFirst, const u32* waveCount)
{
    __shared__ u32 poolMem[NPOOL][LZ_HC_REGION_WORDS];
    __shared__ u32 poolMask;
    for (u32 i = threadIdx.x; i < (u32)NPOOL * LZ_HC_REGION_WORDS; i += blockDim.x) (&poolMem[0][0])[i] = 0x3C3C3C3Cu;
    if (threadIdx.x == 0) poolMask = 0;
    __syncthreads();
    LzHufPool pool; pool.base = &poolMem[0][0]; pool.mask = &poolMask; pool.count = (u32)NPOOL; pool.stride = LZ_HC_REGION_WORDS;
    const u32 lane = lz_lane();
    const u32 w = lz_uniform(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const u32 first = lz_uniform(waveFirst[w]), count = lz_uniform(waveCount[w]);
    for (u32 k = 0; k < count; k++) {
        lz_converge();
        const Job& J = jobs[first + k];
        const u8* const src = (const u8*)lz_uniform64((u64)J.src);
        u8* const out = (u8*)lz_uniform64((u64)J.out);
        const u32 n = lz_uniform(J.n);
        LzStreams st;
        LzHc hc;
        lz_hc_begin(hc, (void*)lz_uniform64((u64)J.slot), lz_uniform(J.maxBlock), lz_uniform(J.searchNum));
        lz_hc_build<SEARCHLEN, HLOG>(src, n, hc, pool, st);
        hc.pre = PRE;
        if constexpr (PRE) lz_hc_hits(src, n, hc); else lz_hc_hits_plain(src, n, hc);
        const u32 nIns = n >= 8u ? n - 7u : 0u;
        for (u32 i = lane; i < (nIns + 63u) / 64u; i += 64u) ((u64*)out)[i] = hc.hits[i];
        for (u32 i = lane; i < nIns; i += 64u) {
            ((u16*)(out + out_prev_at(nIns)))[i] = hc.prev[i];
            ((u32*)(out + out_chain2_at(nIns)))[i] = hc.chain2[i];
            if constexpr (PRE) ((u32*)(out + out_best_at(nIns)))[i] = hc.best[i];
        }
        lz_wave_sync();
        lz_converge();
    }
}

namespace {
const size_t kGuard = 64;
const uint8_t kCanary = 0xC3, kSlotFill = 0xB7;
int g_cases, g_bad;

void mismatch(const char* form, const std::string& name, const char* what, size_t at, uint64_t got, uint64_t want)
{
    if (g_bad++ < 30) fprintf(stderr, "hc_build_kernels: %s %s: %s: at %zu got %llu, want %llu\n", form, name.c_str(), what, at, (unsigned long long)got, (unsigned long long)want);
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Dev {
    uint8_t* base = nullptr; size_t n = 0;
    explicit Dev(size_t bytes) : n(bytes) { CK(hipMalloc((void**)&base, n + 2 * kGuard)); CK(hipMemset(base, kCanary, n + 2 * kGuard)); }
    Dev(const Dev&) = delete;
    ~Dev() { CK(hipFree(base)); }
    uint8_t* p() const { return base + kGuard; }
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

struct Case { std::string name; std::vector<uint8_t> data; uint32_t hasRepeat; };
struct JobDef { uint32_t ci, vi, searchLen, hashLog, searchNum, pre, level; };
struct Model { std::vector<uint16_t> prev; std::vector<uint32_t> two, first; std::vector<uint8_t> hit, open; };

void load(const char* path, std::vector<Case>& cases, std::vector<JobDef>& jobs)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "hc_build_kernels: cannot open %s\n", path); exit(2); }
    auto need = [&](void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "hc_build_kernels: %s is truncated\n", path); exit(2); } };
    char magic[4]; uint32_t nc, nj;
    need(magic, 4); need(&nc, 4); need(&nj, 4);
    if (memcmp(magic, "HCBI", 4) || !nc || nc > 10000u || !nj || nj > 100000u) { fprintf(stderr, "hc_build_kernels: %s is not a case file\n", path); exit(2); }
    cases.resize(nc); jobs.resize(nj);
    for (Case& c : cases) {
        uint32_t h[3];
        need(h, sizeof h);
        if (h[0] > 256u || h[1] > (4u << 20) || h[2] > 1u) { fprintf(stderr, "hc_build_kernels: bad record in %s\n", path); exit(2); }
        c.name.resize(h[0]); c.data.resize(h[1]); c.hasRepeat = h[2];
        need(&c.name[0], h[0]); need(c.data.data(), h[1]);
    }
    for (JobDef& j : jobs) {
        need(&j, sizeof j);
        const bool form = (j.searchLen == 5 && (j.hashLog == 18 || j.hashLog == 14) && !j.pre) || (j.searchLen == 4 && j.hashLog == 18 && j.pre);
        if (j.ci >= nc || !form || !j.searchNum || j.searchNum > 256u) { fprintf(stderr, "hc_build_kernels: bad job in %s\n", path); exit(2); }
    }
    fclose(f);
}

uint32_t n_ins(size_t n) { return n >= 8 ? (uint32_t)n - 7u : 0u; }
size_t slot_bytes(size_t maxBlock, bool pre)
{
    const size_t cap = (maxBlock + 65535u) & ~(size_t)65535u;
    return LZ_HC_SLOT_BYTES(cap) - (pre ? 0u : 4u * cap);
}

const Model& model_of(const std::vector<Case>& cases, const JobDef& j)
{
    static std::map<std::pair<uint32_t, uint32_t>, Model> cache;
    auto key = std::make_pair(j.ci, j.level);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    Model& m = cache[key];
    const std::vector<uint8_t>& d = cases[j.ci].data;
    const uint32_t nIns = n_ins(d.size());
    m.prev.resize(nIns + 1); m.two.resize(nIns + 1); m.hit.resize(nIns + 1); m.first.resize(nIns + 1); m.open.resize(nIns + 1);
    const uint8_t none = 0;
    const int r = lzo_hc_tables(d.empty() ? &none : d.data(), (int)d.size(), (int)j.level, m.prev.data(), m.two.data(), m.hit.data(), m.first.data(), m.open.data());
    if (r != (int)nIns) { fprintf(stderr, "hc_build_kernels: lzo_hc_tables(%s, level %u) returned %d\n", cases[j.ci].name.c_str(), j.level, r); exit(2); }
    return m;
}

void compare(const char* form, const std::vector<Case>& cases, const JobDef& j, const uint8_t* out)
{
    const Case& c = cases[j.ci];
    const std::string name = c.name + "/n" + std::to_string(j.searchNum) + "_h" + std::to_string(j.searchLen) + "_" + std::to_string(j.hashLog);
    const Model& m = model_of(cases, j);
    const uint32_t nIns = n_ins(c.data.size());
    const uint64_t* hits = (const uint64_t*)out;
    const uint16_t* prev = (const uint16_t*)(out + out_prev_at(nIns));
    const uint32_t* chain2 = (const uint32_t*)(out + out_chain2_at(nIns));
    const uint32_t* best = (const uint32_t*)(out + out_best_at(nIns));
    const int before = g_bad;
    size_t decidedNonZero = 0;
    for (uint32_t p = 0; p < nIns && g_bad == before; p++) {
        if (prev[p] != m.prev[p]) mismatch(form, name, "prev", p, prev[p], m.prev[p]);
        else if (chain2[p] != m.two[p]) mismatch(form, name, "chain2", p, chain2[p], m.two[p]);
        else if (((hits[p >> 6] >> (p & 63u)) & 1u) != m.hit[p]) mismatch(form, name, "hit bit", p, (hits[p >> 6] >> (p & 63u)) & 1u, m.hit[p]);
        else if (j.pre) {
            if (best[p] == LZ_HC_BEST_OPEN) { if (!m.open[p]) mismatch(form, name, "best is open where the model decides", p, best[p], m.first[p]); }
            else if (best[p] != m.first[p]) mismatch(form, name, "best", p, best[p], m.first[p]);
            else decidedNonZero += best[p] != 0u;
        }
    }
    if (nIns & 63u) { const uint64_t tail = hits[nIns >> 6] >> (nIns & 63u); if (tail) mismatch(form, name, "hit bits at and beyond nIns", nIns, tail, 0); }
    if (j.pre && c.hasRepeat && g_bad == before && !decidedNonZero) mismatch(form, name, "no decided non-zero entry of best", 0, 0, 1);
    g_cases++;
}

typedef void (*Kernel)(const Job*, const u32*, const u32*);
Kernel kernel_of(const JobDef& j, int npool)
{
    if (j.pre) return npool == LZ_HC_POOL ? hc_tables_kernel<4, 18, true, LZ_HC_POOL> : hc_tables_kernel<4, 18, true, LZ_HC_POOL + 1>;
    if (j.hashLog == 14) return npool == LZ_HC_POOL ? hc_tables_kernel<5, 14, false, LZ_HC_POOL> : hc_tables_kernel<5, 14, false, LZ_HC_POOL + 1>;
    return npool == LZ_HC_POOL ? hc_tables_kernel<5, 18, false, LZ_HC_POOL> : hc_tables_kernel<5, 18, false, LZ_HC_POOL + 1>;
}
int class_of(const JobDef& j) { return j.pre ? 1 : j.hashLog == 14 ? 2 : 0; }

// The sources in one device buffer, each behind a 16-byte boundary with a gap to the next
struct Sources {
    std::vector<size_t> at; std::vector<uint8_t> host;
    explicit Sources(const std::vector<Case>& cases)
    {
        size_t cur = 0;
        for (const Case& c : cases) { at.push_back(align_up(cur, 16)); cur = at.back() + c.data.size() + 64; }
        host.assign(cur, 0x5A);
        for (size_t i = 0; i < cases.size(); i++) if (!cases[i].data.empty()) memcpy(&host[at[i]], cases[i].data.data(), cases[i].data.size());
    }
};

// One form over the jobs of one kernel class.  waves: the jobs (indices into `jobs`) of each wave, in the order it runs them;
// wavesPerGroup consecutive waves make a workgroup.  A wave's slot is laid out for its FIRST job's size.
void run_form(const char* form, const std::vector<Case>& cases, const std::vector<JobDef>& jobs, const Sources& S, const Dev& dSrc,
              const std::vector<std::vector<uint32_t>>& waves, uint32_t wavesPerGroup, int npool)
{
    const JobDef* first0 = nullptr;
    for (const auto& v : waves) if (!v.empty()) { first0 = &jobs[v[0]]; break; }
    if (!first0 || waves.size() % wavesPerGroup) return;
    const JobDef& j0 = *first0;
    const bool pre = j0.pre != 0;
    std::vector<Job> tab; std::vector<uint32_t> order, first, count;
    std::vector<size_t> slotAt, slotLen, outAt;
    std::vector<std::string> slotName;
    size_t slotCur = 0, outCur = 0;
    const uint32_t nGroups = (uint32_t)(waves.size() / wavesPerGroup);
    for (uint32_t w = 0; w < waves.size(); w++) {
        first.push_back((uint32_t)tab.size());
        count.push_back((uint32_t)waves[w].size());
        if (waves[w].empty()) continue;                            // a wave without work
        const size_t maxBlock = std::max<size_t>(cases[jobs[waves[w][0]].ci].data.size(), 1);
        slotAt.push_back(slotCur + kGuard); slotLen.push_back(slot_bytes(maxBlock, pre)); slotName.push_back(cases[jobs[waves[w][0]].ci].name);
        slotCur = align_up(slotAt.back() + slotLen.back() + kGuard, 256);
        for (uint32_t ji : waves[w]) {
            const JobDef& j = jobs[ji];
            const size_t n = cases[j.ci].data.size();
            if (n > maxBlock || class_of(j) != class_of(j0)) { fprintf(stderr, "hc_build_kernels: bad wave\n"); exit(2); }
            Job J; J.src = nullptr; J.slot = nullptr; J.out = nullptr; J.n = (u32)n; J.maxBlock = (u32)maxBlock; J.searchNum = j.searchNum; J.pad = (u32)(slotAt.size() - 1);
            outAt.push_back(outCur); outCur = align_up(outCur + out_bytes(n_ins(n), pre) + 64, 64);
            tab.push_back(J); order.push_back(ji);
        }
    }
    Dev dSlots(slotCur), dOut(outCur), dJobs(tab.size() * sizeof(Job)), dFirst(first.size() * 4), dCount(count.size() * 4);
    for (size_t s = 0; s < slotAt.size(); s++) CK(hipMemset(dSlots.p() + slotAt[s], kSlotFill, slotLen[s]));
    for (size_t i = 0; i < tab.size(); i++) {
        tab[i].src = dSrc.p() + S.at[jobs[order[i]].ci]; tab[i].slot = dSlots.p() + slotAt[tab[i].pad]; tab[i].out = dOut.p() + outAt[i]; tab[i].pad = 0;
    }
    dJobs.put(tab.data()); dFirst.put(first.data()); dCount.put(count.data());
    hipLaunchKernelGGL(kernel_of(j0, npool), dim3(nGroups), dim3(64 * wavesPerGroup), 0, 0, (const Job*)dJobs.p(), (const u32*)dFirst.p(), (const u32*)dCount.p());
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    const std::vector<uint8_t> out = dOut.get(form, "tables");
    for (size_t i = 0; i < tab.size(); i++) compare(form, cases, jobs[order[i]], out.data() + outAt[i]);
    // the canaries around every slot (the arena starts as canary bytes; only the slots were filled)
    std::vector<uint8_t> g(2 * kGuard);
    for (size_t s = 0; s < slotAt.size(); s++) {
        CK(hipMemcpy(g.data(), dSlots.p() + slotAt[s] - kGuard, kGuard, hipMemcpyDeviceToHost));
        CK(hipMemcpy(g.data() + kGuard, dSlots.p() + slotAt[s] + slotLen[s], kGuard, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * kGuard; i++) if (g[i] != kCanary) { mismatch(form, slotName[s], i < kGuard ? "canary in front of the slot" : "canary behind the slot", i % kGuard, g[i], kCanary); break; }
    }
    if (dJobs.get(form, "job table") != std::vector<uint8_t>((uint8_t*)tab.data(), (uint8_t*)(tab.data() + tab.size()))) mismatch(form, "job table", "changed", 0, 1, 0);
    if (dSrc.get(form, "sources") != S.host) mismatch(form, "sources", "the source bytes changed", 0, 1, 0);
}
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: hc_build_kernels CASEFILE\n"); return 2; }
    std::vector<Case> cases; std::vector<JobDef> jobs;
    load(argv[1], cases, jobs);
    const Sources S(cases);
    Dev dSrc(S.host.size());
    dSrc.put(S.host.data());
    for (int cls = 0; cls < 3; cls++) {
        std::vector<uint32_t> mine;                                // this class's jobs, the largest first
        for (uint32_t i = 0; i < jobs.size(); i++) if (class_of(jobs[i]) == cls) mine.push_back(i);
        std::stable_sort(mine.begin(), mine.end(), [&](uint32_t a, uint32_t b) { return cases[jobs[a].ci].data.size() > cases[jobs[b].ci].data.size(); });
        if (mine.empty()) continue;
        std::vector<std::vector<uint32_t>> alone, sixteen, rows;
        for (uint32_t i : mine) alone.push_back({ i });
        // (b): wave w of group g = job g + w * nGroups of the sorted list (none behind its end): every group gets large and small ones
        const size_t nGroups = (mine.size() + LZ_WAVES_HC - 1) / LZ_WAVES_HC;
        for (size_t g = 0; g < nGroups; g++)
            for (size_t w = 0; w < LZ_WAVES_HC; w++) {
                sixteen.push_back({});
                if (g + w * nGroups < mine.size()) sixteen.back().push_back(mine[g + w * nGroups]);
            }
        run_form("(a) alone in a workgroup", cases, jobs, S, dSrc, alone, 1, LZ_HC_POOL + 1);
        run_form("(b) sixteen waves, three regions", cases, jobs, S, dSrc, sixteen, LZ_WAVES_HC, LZ_HC_POOL);
        // (c): row r = jobs r, r + nRows, r + 2 nRows, ... of the sorted list: eight in a row, the largest first
        const size_t nRows = (mine.size() + 7) / 8;
        for (size_t r = 0; r < nRows; r++) { rows.push_back({}); for (size_t k = r; k < mine.size(); k += nRows) rows.back().push_back(mine[k]); }
        run_form("(c) eight in a row through one slot", cases, jobs, S, dSrc, rows, 1, LZ_HC_POOL + 1);
    }
    printf("cases: %d mismatches: %d\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
