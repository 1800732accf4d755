"""CPU: the source read-ahead of the level-10 producers (lizard_amd/csrc/lz_touch.h, lz_parse_fast LANEFORMS) on the SIMT emulator,
with the log hook of the touch's host form installed (tests/emul/readahead_api.cpp): every touch and every round's first position,
per block.  Blocks: tests/source_readahead_inputs.py — 21 .. 262 144 bytes of P50 and of noise, one 515-byte-period repeat, and a
ragged batch of blocks at odd addresses whose last block ends at the last byte of the area.

Asserted per block:
  1. the bytes of every touch (LZ_RA_BYTES at byte LZ_RA_AT of a line of the absolute address) lie inside [src, src + n) of its own block;
  2. the touched lines ascend without a gap from the first line that starts inside the block (so no line is touched twice), and every
     round keeps the rule: at most LZ_RA_PER_ROUND touches, no line at or beyond min(p0 + LZ_READAHEAD, the last line whose touch fits
     into the block), and behind its touches the cursor stands at that limit or the round used all its touches;
  3. the cursor is complete — every line that starts in the block and whose touch fits into it was touched — on the P50 blocks, the data the read-ahead is
     for: a winner every 110 bytes restarts the visit schedule, a round seldom moves on by more than the LZ_RA_PER_ROUND lines it may
     ask for, and the last LZ_READAHEAD bytes of a block take several rounds.  It is NOT complete, and cannot be under a limit per
     round, where rounds outrun that limit for good: noise (a run without a winner visits every k-th byte in its k-th round, 64 k bytes
     per round) and the 515-byte-period block (its parse ends behind a match of 130 KiB; the bytes inside a match are read by the
     count trips and nobody waits for them again).  There the rule of 2. is all that holds, and the test prints how far the cursor came;
  4. the output is the oracle's.
The stand-alone program tests/readahead_asan_main.cpp runs the same blocks under AddressSanitizer with sources of exactly n bytes."""
import ctypes
import os
import re
import subprocess

import pytest

import source_readahead_inputs as inputs
import util

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
CSRC = os.path.join(util.ROOT, "lizard_amd", "csrc")


def _lib():
    """tests/emul/libreadahead_emul.so from simt.cpp + readahead_api.cpp, the way tests/emul/build.py builds libemul.so."""
    out = os.path.join(EMUL, "libreadahead_emul.so")
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "readahead_api.cpp")]
    deps = srcs + [os.path.join(EMUL, "lz_wave.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + srcs)
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.emul_readahead_split.restype = ctypes.c_long
    L.emul_readahead_split.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_long]
    return L


@pytest.fixture(scope="module")
def emu():
    return _lib()


@pytest.fixture(scope="module")
def knobs(emu):
    k = (ctypes.c_uint * 6)()
    emu.emul_readahead_knobs(k)
    on, ahead, line, per_round, at, width = (int(x) for x in k)
    assert on == 1, "the tree builds the level-10 producers without the read-ahead: nothing to check"
    assert line in (64, 128) and ahead >= 516 + line and per_round >= 1 and at % 4 == 0 and at + width <= line + 4
    return ahead, line, per_round, at, width


def run(emu, area, blocks, nprod=1, ncons=1, seed=1):
    """The batch `blocks` = [(offset, size)] of `area` through the emulated split kernel.  Returns (outputs, events per block): an
    event is ("round", p0) or ("touch", absolute aligned address), in the order the block's producer made them."""
    nb = len(blocks)
    src = ctypes.create_string_buffer(bytes(area), len(area))
    base = ctypes.addressof(src)
    offs = (ctypes.c_ulonglong * nb)(*[o for o, _ in blocks])
    sizes_in = (ctypes.c_uint * nb)(*[n for _, n in blocks])
    stride = util.oracle().lzo_compress_bound(max(n for _, n in blocks)) + 64
    dst = ctypes.create_string_buffer(nb * stride)
    sizes = (ctypes.c_uint * nb)()
    cap = 64 + sum(n // 16 + 64 for _, n in blocks)                 # (a round moves on by a byte at least, a touch by a line)
    log = (ctypes.c_ulonglong * (2 * cap))()
    got = emu.emul_readahead_split(src, nb, offs, sizes_in, dst, stride, sizes, inputs.LEVEL, nprod, ncons, seed, log, cap)
    assert 0 <= got <= cap, (got, cap)
    events = {base + o: [] for o, _ in blocks}
    for i in range(got):
        b, w = int(log[2 * i]), int(log[2 * i + 1])
        assert b in events, "a touch names a block that is not in the batch"
        off, what = w & 0xFFFFFFFF, w >> 32
        events[b].append(("round", off) if what else ("touch", (b + off) & ~3))
    outs = [dst.raw[i * stride:i * stride + sizes[i]] for i in range(nb)]
    return outs, [(base + o, n, events[base + o]) for o, n in blocks]


def check_block(src, n, events, knobs, complete, what):
    """Assertions 1 to 3 of the module's text for one block at address src.  Returns (lines touched, lines that could be)."""
    ahead, line, per_round, at, width = knobs
    end = n - (at + width) + 1 if n >= at + width else 0            # a line that starts at an offset below it may be touched
    start0 = src + (-src) % line                                    # the first line that starts inside the block
    lines, in_round, p0, cursor = [], 0, None, start0 - src
    def close_round():
        if p0 is not None:
            lim = min(p0 + ahead, end)
            assert in_round <= per_round, (what, "touches in one round", in_round)
            assert in_round == per_round or cursor >= lim, (what, "a round stopped short of its limit", p0, cursor, lim)
    for kind, v in events:
        if kind == "round":
            close_round()
            p0, in_round = v, 0
            continue
        assert src <= v and v + width <= src + n, (what, "touch outside the block", v - src, n)                   # 1.
        start = v - at
        assert start == (lines[-1] + line if lines else start0), (what, "lines ascend one by one from the block's first", start - src)    # 2.
        assert p0 is not None and start - src < min(p0 + ahead, end), (what, "touch beyond the round's limit", start - src, p0)
        in_round += 1
        lines.append(start)
        cursor = start + line - src                                 # the first untouched line
    close_round()
    possible = len(range(start0 - src, end, line))
    if complete:
        assert len(lines) == possible, (what, "the cursor did not reach the block's end", len(lines), possible)   # 3.
    return len(lines), possible


def test_every_block_alone(emu, knobs):
    """Each block as a launch of its own; the coverage of the blocks that outrun the cursor is printed."""
    for case, (name, data, outruns) in enumerate(inputs.all_blocks()):
        outs, per_block = run(emu, data, [(0, len(data))], seed=case + 1)
        assert outs == [inputs.expected(data)], name                                                             # 4.
        (src, n, events), = per_block
        touched, possible = check_block(src, n, events, knobs, not outruns, name)
        if outruns:
            print("%s: %d of %d lines touched in %d rounds" % (name, touched, possible, sum(1 for k, _ in events if k == "round")))
    name, data, _ = inputs.all_blocks()[-1]
    assert name.startswith("repeat515") and touched < possible, "the block meant to outrun the cursor did not"


def test_ragged_batch_at_odd_addresses(emu, knobs):
    """Blocks at odd addresses, the last one ending at the area's last byte, over two producers (every producer takes several blocks:
    the cursor starts anew with each) and over one."""
    area, blocks = inputs.ragged_area()
    for nprod, seed in ((2, 5), (1, 6)):
        outs, per_block = run(emu, area, blocks, nprod=nprod, seed=seed)
        for (o, n), out, (src, _, events) in zip(blocks, outs, per_block):
            assert out == inputs.expected(area[o:o + n]), (nprod, o, n)
            assert src % 2 == 1
            check_block(src, n, events, knobs, True, ("ragged", nprod, o, n))


def test_same_blocks_under_address_sanitizer(tmp_path):
    """tests/readahead_asan_main.cpp as a program of its own: the same sizes and kinds with sources of exactly n bytes, and a ragged
    batch whose last block ends at the last byte of its allocation; exit status 0, no report, every output the oracle's."""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    cxx = ["-std=c++17", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread"]
    probe = subprocess.run(["g++", "-x", "c++", "-", "-fsanitize=address,undefined", "-o", os.devnull], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    if probe.returncode:
        pytest.skip("no AddressSanitizer / UndefinedBehaviorSanitizer runtime")
    jobs = [(["gcc", "-std=gnu99"], os.path.join(util.ORACLE_DIR, "lizard_oracle.c")),
            (["gcc", "-std=gnu99"], os.path.join(util.ORACLE_DIR, "huf_oracle.c")),
            (["g++"] + cxx + ["-I", EMUL], os.path.join(EMUL, "simt.cpp")),
            (["g++"] + cxx + ["-I", EMUL], os.path.join(EMUL, "readahead_api.cpp")),
            (["g++"] + cxx, os.path.join(HERE, "readahead_asan_main.cpp"))]
    procs, objs = [], []
    for cmd, src in jobs:
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        procs.append(subprocess.Popen(cmd + san + ["-c", src, "-o", objs[-1]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    for p in procs:
        log = p.communicate()[0]
        assert p.returncode == 0, "the sanitized program does not build:\n" + log[-3000:]
    exe = str(tmp_path / "readahead_asan_main")
    subprocess.run(["g++"] + san + ["-pthread"] + objs + ["-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    m = re.fullmatch(r"cases: (\d+) mismatches: (\d+) touches: (\d+)", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(2)) == 0 and int(m.group(3)) > 0, tail
    assert int(m.group(1)) == 2 * len(inputs.SIZES) + 1 + 2, tail
