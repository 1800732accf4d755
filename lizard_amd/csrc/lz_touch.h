// lz_touch.h — source read-ahead of the level-10 producers: a load whose only purpose is to bring a source line into the XCD's L2
// before the parse reads it (lz_parse_fast, LANEFORMS).  Included by lz_block.h behind lz_wave.h.
//
// Why a SCALAR load.  gfx950 returns a wave's vector loads in order through one vmcnt: a read-ahead issued as a vector load stands
// in the same queue as the round's candidate batch, and every later counted wait of the round waits for its HBM trip as well
// (tools/probes/readahead_probe.hip, "behind-cold": an L2 hit issued behind a first touch costs the first touch).  Scalar loads
// return out of order, are counted in lgkmcnt, and fill the L2 on the way.  What the probe measured (profiles/source_readahead_probe.txt,
// 13 waves per CU): a first touch by the vector path 1 100 clocks, an L2 hit 350, the line after a scalar touch of BOTH its 64-byte
// halves 300.  A scalar request fills 64 bytes and the vector L1 asks the L2 for whole 128-byte lines: after ONE scalar dword per
// 128-byte line the vector load still costs a first touch (920), also when it stays inside the touched half.  Hence two forms:
//   LZ_RA_LINE 128   one 8-byte scalar load across the middle of the line (bytes 60..67): one instruction, two requests, and the
//                    line then costs 300 to 330 clocks like the one below;
//   LZ_RA_LINE 64    one dword at the start of every 64-byte half: twice the instructions, +0.7 % on the headline where the form
//                    above gives +2.6 % (profiles/source_readahead_ab.txt) — the producers' loop is short of issue slots.
//
// lz_touch(base, off): base + off is dword-aligned and wave-uniform (the cursor stands on lines of the ABSOLUTE address).  The value
// is handed back and must reach lz_touch_use() behind a wait the wave makes anyway (the exchange's lgkmcnt(0), one round later): it
// is never used for a decision, the hand-back only keeps the compiler from putting a wait of its own right behind the load.
// Host form (test emulator, sanitizer builds): a real read of the same bytes, so that a touch outside the block is an out-of-bounds
// read there, and a thread-local hook that receives every touch (lane 0's call) and every round's position.
#pragma once
#ifndef LZ_SRC_READAHEAD
#define LZ_SRC_READAHEAD 1                                   // 0: the producers' loop without the read-ahead (profiles/source_readahead_ab.txt)
#endif
#ifndef LZ_READAHEAD
#define LZ_READAHEAD 1024u                                   // bytes in front of the round's first position that are requested; covers
#endif                                                       // the count trip's reach (P + 516) plus the progress of one loaded HBM trip
#ifndef LZ_RA_LINE
#define LZ_RA_LINE 128u
#endif
#ifndef LZ_RA_PER_ROUND
#define LZ_RA_PER_ROUND 2u                                   // touches per round at most: 256 bytes, a round moves on by about 110
#endif
#if LZ_RA_LINE == 128
#define LZ_RA_AT    60u                                      // where in its line a touch reads, and how many bytes
#define LZ_RA_BYTES 8u
#else
#define LZ_RA_AT    0u
#define LZ_RA_BYTES 4u
#endif

struct LzTouched { u32 a, b; };                              // what a touch hands back (b: the 8-byte form only)

#if defined(__HIPCC__)
LZ_DEV LzTouched lz_touch(const u8* base, u32 off)
{
    const uintptr_t a = ((uintptr_t)base + off) & ~(uintptr_t)3;
    LzTouched t = { 0u, 0u };
#if LZ_RA_BYTES == 8
    typedef u32 lz_u32x2 __attribute__((ext_vector_type(2)));
    typedef lz_u32x2 __attribute__((aligned(4))) lz_u32x2_a4;
    const lz_u32x2_a4 v = __builtin_nontemporal_load((const __attribute__((address_space(4))) lz_u32x2_a4*)a);
    t.a = v.x; t.b = v.y;
#else
    t.a = __builtin_nontemporal_load((const __attribute__((address_space(4))) u32*)a);
#endif
    return t;
}
LZ_DEV void lz_touch_use(const LzTouched& t) { asm volatile("" :: "s"(t.a), "s"(t.b)); }
LZ_DEV void lz_touch_round(const u8*, u32) {}
#else
// what: 0 = a touch of LZ_RA_BYTES bytes at base + off, 1 = a round of the parse whose first position is off
typedef void (*lz_touch_hook_t)(const u8* base, u32 off, int what);
inline thread_local lz_touch_hook_t lz_touch_hook = nullptr;
LZ_DEV LzTouched lz_touch(const u8* base, u32 off)
{
    const uintptr_t a = ((uintptr_t)base + off) & ~(uintptr_t)3;
    if (lz_touch_hook && lz_lane() == 0) lz_touch_hook(base, off, 0);
    LzTouched t = { 0u, 0u };
    memcpy(&t, (const void*)a, LZ_RA_BYTES);
    return t;
}
LZ_DEV void lz_touch_use(const LzTouched& t) { asm volatile("" :: "r"(t.a), "r"(t.b)); }
LZ_DEV void lz_touch_round(const u8* base, u32 p0) { if (lz_touch_hook && lz_lane() == 0) lz_touch_hook(base, p0, 1); }
#endif

// The cursor of one block (LzStreams::raAt / raEnd, set by lz_split_producer): raAt is the offset of the next line to touch — the
// block's lines are those of the absolute address that START inside it — and raEnd the first offset at which a line may not be
// touched any more: the bytes of a touch lie inside [src, src + n) of the BLOCK, whatever the sub-block, the batch's stride or the
// neighbouring block are.  (The bytes in front of the block's first line boundary are the first ones the parse reads: nothing
// could be ahead of that.)
LZ_DEV void lz_touch_begin(const u8* src, u32 n, u32& raAt, u32& raEnd)
{
    raAt = (0u - (u32)(uintptr_t)src) & (LZ_RA_LINE - 1u);
    raEnd = n >= LZ_RA_AT + LZ_RA_BYTES ? n - (LZ_RA_AT + LZ_RA_BYTES) + 1u : 0u;
}
