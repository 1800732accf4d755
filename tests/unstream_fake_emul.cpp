// tests/unstream_fake_emul.cpp — TEST INFRASTRUCTURE ONLY: the body of lz_unstream_walk_kernel (lizard_amd/csrc/unstream_kernels.h, with
// lz_unframe_walk inside it) on the CPU SIMT emulator, for tests/unstream_device_fake.c: the fake device's stream-walk "kernel" runs the
// very code the GPU runs, so the host file is tested against it and not against a restatement.  Linked beside
// tests/pipeline_fake_emul.cpp, which defines lzemu_stats; the closure that calls this checks the ranges against the fake device's
// allocations.
#include "lz_wave.h"            // tests/emul/lz_wave.h (emulator) — must come first
#include "../lizard_amd/csrc/unstream_kernels.h"

namespace {
struct StreamArgs { const u8* src; u64 srcSize; LzStreamCtl* ctl; LzWalkResult* res; u64* offs; u32 tableCap; };
void entry_stream(void* a) { StreamArgs* x = (StreamArgs*)a; lz_unstream_walk(x->src, x->srcSize, x->ctl, x->res, x->offs, x->tableCap); }
}  // namespace

extern "C" void emul_unstream_segment(const void* src, unsigned long long srcSize, void* ctl, void* res, unsigned long long* offs, unsigned tableCap,
                                      unsigned seed)
{
    StreamArgs a = { (const u8*)src, srcSize, (LzStreamCtl*)ctl, (LzWalkResult*)res, (u64*)offs, tableCap };
    lzemu::run_wave(entry_stream, &a, seed);
}
