"""Where the compress kernels write: LizardGPU_compressBlocks_device at the documented minimum stride, and the host entries at
their exact capacity.

The bound is tight — an incompressible block ends 1 byte below Lizard_compressBound(n), 5 bytes below it where 128 KiB divides n —
and the kernels copy with 4-, 8- and 16-byte stores whose last piece is pulled back to end exactly.  api.compress_blocks_device
rounds the stride up to 64, so a piece that is not pulled back lands in slack there.  Here the slots are bound(blockSize) + P bytes
apart, P = 0 (the minimum of include/lizard_amd.h), 1 and 61, at odd byte offsets inside one tensor of 0xC3:

    | 4 KiB margin | off | slot 0 | P | slot 1 | P | ... | slot nb-1 | P | rest + 4 KiB margin |

and after one synchronise the margins, every P-byte pad, the sentinel words around `sizes` and the source must be untouched, every
size within 1 .. bound(n_i) and the first sizes[i] bytes of every slot the oracle's.  With P = 0 an overrun lands in the
neighbouring slot: it shows as a wrong byte there when the overrunning wave wrote last, or in the margin behind the last slot; with
P > 0 it shows in the pad whoever wrote last.  Blocks alternate incompressible / one run / text-like, so neighbours finish at
different times and end at different distances from the bound; the CPU test at the top checks with the oracle that the incompressible
ones do end where this paragraph says, at every level and size used.

Reads past the end of the source are the business of tests/test_emulator_asan.py, on the CPU.
"""
import functools

import numpy as np
import pytest

import util

LEVELS = (10, 30, 11, 31, 12, 32, 13, 16, 35, 37, 20, 40, 21, 41, 22, 42)    # one per kernel instantiation
SMALL = (1, 19, 21, 4097)                # nb = 2 x resident waves + 3: several blocks per wave, every slot reused
LARGE = (65537, 131072, 131073)          # nb = 67: fewer blocks than the machine, the launch is spread (LzBatch::activeWaves)
HUGE = (4 << 20) + 1                     # nb = 3, levels 10 / 30: a block above 4 MiB
MARGIN = 4096
CANARY = 0xC3
SRC_FILL = 0x5A
SENTINEL = 0xA5A5A5A5
KINDS = ("noise", "run", "text")
SENTENCE = np.frombuffer(b"the quick brown fox jumps over the lazy dog; pack my box with five dozen liquor jugs. ", dtype=np.uint8)


def bound(n):
    return n + 2 + 4 * (n // 131072 + 1)           # Lizard_compressBound, lib/lizard_compress.h:124


@functools.lru_cache(maxsize=None)
def block(kind, variant, n):
    """Block contents by kind; three variants of the kinds that have any.  Read-only arrays, shared by every test."""
    rs = np.random.RandomState(1000 * KINDS.index(kind) + 10 * variant + 1)
    if kind == "noise":
        a = rs.randint(0, 256, n).astype(np.uint8)
    elif kind == "run":
        a = np.full(n, 0x41 + variant, dtype=np.uint8)
    else:
        a = np.resize(np.roll(SENTENCE, variant), n).copy()
        breaks = np.cumsum(rs.randint(1, 600, n // 300 + 1))
        breaks = breaks[breaks < n]
        a[breaks] = rs.randint(0, 256, len(breaks))
    a.setflags(write=False)
    return a


def kind_of(i):
    return KINDS[i % 3], (i // 3) % 3


@functools.lru_cache(maxsize=None)
def expected(kind, variant, n, level):
    """The oracle's bytes, computed once per distinct block."""
    out = np.frombuffer(util.oracle_compress(block(kind, variant, n).tobytes(), level), dtype=np.uint8)
    assert 1 <= len(out) <= bound(n)
    return out


def sizes_for(level):
    return SMALL + LARGE + ((HUGE,) if level in (10, 30) else ())


# ---------------------------------------------------------------- CPU: the inputs are at the edge ------------------------------

@pytest.mark.parametrize("level", LEVELS)
def test_incompressible_blocks_end_at_the_bound(level):
    """Every level's container stores an incompressible block raw: the level byte, then per 128 KiB sub-block a 4-byte header and
    the bytes.  That is bound(n) - 1, or bound(n) - 5 where 128 KiB divides n (the bound counts one sub-block more)."""
    assert util.oracle().lzo_compress_bound(HUGE) == bound(HUGE)
    for n in sizes_for(level) + tuple(s - 1 for s in LARGE):
        assert util.oracle().lzo_compress_bound(n) == bound(n)
        for variant in ((0, 1, 2) if n < HUGE else (0,)):
            got = len(expected("noise", variant, n, level))
            print("level %d n %d variant %d: %d of %d" % (level, n, variant, got, bound(n)))
            assert got == bound(n) - (5 if n % 131072 == 0 else 1), (level, n, variant)
    # ... and the other kinds end well below it (neighbours at different distances from the bound)
    for n in (4097, 131073):
        assert len(expected("run", 0, n, level)) < n // 8 and len(expected("text", 0, n, level)) < n // 2, (level, n)


# ---------------------------------------------------------------- GPU -------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  (before the library: one HIP runtime per process, torch's)
    from lizard_amd import _lib
    return _lib.lib()      # raises loudly if the HIP extension is not built


def make_source(nb, block_size, last):
    """(host array of the blocks back to back, [(kind, variant, n)] per block)"""
    what = [kind_of(i) + (block_size if i < nb - 1 else last,) for i in range(nb)]
    src = np.empty((nb - 1) * block_size + last, dtype=np.uint8)
    for i, (kind, variant, n) in enumerate(what):
        src[i * block_size:i * block_size + n] = block(kind, variant, n)
    return src, what


def run_device_case(L, level, block_size, nb, last, P, off, compare):
    """One launch, one synchronise, then every assertion of the module's docstring.  `compare`: the blocks whose bytes are compared
    with the oracle (sizes are checked for all)."""
    import torch
    dev = torch.device("cuda", 0)
    src_host, what = make_source(nb, block_size, last)
    stride = bound(block_size) + P
    src_dev = torch.full((MARGIN + off + len(src_host) + MARGIN,), SRC_FILL, dtype=torch.uint8, device=dev)
    src_dev[MARGIN + off:MARGIN + off + len(src_host)] = torch.from_numpy(src_host).to(dev)
    src_before = src_dev.cpu()
    dst_dev = torch.full((MARGIN + off + nb * stride + MARGIN,), CANARY, dtype=torch.uint8, device=dev)
    first = 17                                              # word 17 of a 256-byte aligned tensor: 4-byte aligned, 4 past a 64-byte line
    sizes_dev = torch.full((first + nb + 16,), SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    assert (sizes_dev.data_ptr() + 4 * first) % 64 == 4
    torch.cuda.synchronize()
    rc = L.LizardGPU_compressBlocks_device(src_dev.data_ptr() + MARGIN + off, nb, block_size, last, dst_dev.data_ptr() + MARGIN + off, stride,
                                           sizes_dev.data_ptr() + 4 * first, level, None)
    torch.cuda.synchronize()
    tag = (level, block_size, nb, last, P, off)
    assert rc == 0, (tag, L.LizardGPU_lastError())
    dst = dst_dev.cpu().numpy()
    words = sizes_dev.cpu().numpy().view(np.uint32)
    # margins, sentinels, source
    assert (dst[:MARGIN + off] == CANARY).all(), ("front margin of dst", tag, np.flatnonzero(dst[:MARGIN + off] != CANARY)[:8])
    back = dst[MARGIN + off + nb * stride:]
    assert (back == CANARY).all(), ("back margin of dst", tag, np.flatnonzero(back != CANARY)[:8])
    assert (words[:first] == SENTINEL).all() and (words[first + nb:] == SENTINEL).all(), ("sentinels around sizes", tag)
    assert torch.equal(src_dev.cpu(), src_before), ("source changed", tag)
    slots = dst[MARGIN + off:MARGIN + off + nb * stride].reshape(nb, stride)
    if P:
        pads = slots[:, bound(block_size):]
        assert (pads == CANARY).all(), ("pad behind a slot", tag, np.argwhere(pads != CANARY)[:8])
    # sizes of every block, bytes of the compared ones: by distinct content, all its blocks at once
    sizes = words[first:first + nb]
    groups = {}
    for i, w in enumerate(what):
        groups.setdefault(w, []).append(i)
    compare = set(compare)
    for (kind, variant, n), idx in groups.items():
        want = expected(kind, variant, n, level)
        idx = np.array(idx)
        assert ((sizes[idx] >= 1) & (sizes[idx] <= bound(n))).all(), ("size outside 1 .. bound", tag, kind, sizes[idx][:8])
        assert (sizes[idx] == len(want)).all(), ("size", tag, kind, variant, n, len(want), idx[sizes[idx] != len(want)][:8], sizes[idx][sizes[idx] != len(want)][:8])
        rows = np.array([i for i in idx if i in compare], dtype=np.int64)
        if len(rows):
            bad = (slots[rows, :len(want)] != want).any(axis=1)
            assert not bad.any(), ("bytes", tag, kind, variant, n, rows[bad][:8])


# (P, off) of the three launches of a case: the minimum stride at every offset once over the module, both pads
LAUNCHES = ((0, 0), (1, 3), (61, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("block_size", SMALL)
@pytest.mark.parametrize("level", LEVELS)
def test_device_batch_small_blocks_exact_stride(L, level, block_size):
    """2 x resident waves + 3 blocks: several per wave, scratch and table slots reused; every block compared."""
    if not L.LizardGPU_levelSupported(level):
        pytest.skip("level %d is not on the GPU path" % level)
    nb = 2 * L.LizardGPU_residentWaves() + 3
    for k, (P, off) in enumerate(LAUNCHES):
        last = (1, block_size, max(1, block_size - 1))[k]
        run_device_case(L, level, block_size, nb, last, P, (off + level) % 4 if P == 0 else off, range(nb))


@pytest.mark.gpu
@pytest.mark.parametrize("block_size", LARGE)
@pytest.mark.parametrize("level", LEVELS)
def test_device_batch_large_blocks_exact_stride(L, level, block_size):
    """67 blocks (the launch is spread over the CUs), a ragged last block of 1 byte and of blockSize - 1; the first, the last and every
    7th block compared."""
    if not L.LizardGPU_levelSupported(level):
        pytest.skip("level %d is not on the GPU path" % level)
    nb = 67
    compare = sorted(set(range(0, nb, 7)) | {0, nb - 1})
    for k, (P, off) in enumerate(LAUNCHES):
        run_device_case(L, level, block_size, nb, (1, block_size - 1, 1)[k], P, off, compare)
    run_device_case(L, level, block_size, nb, block_size - 1, 0, 1 + level % 3, compare)


@pytest.mark.gpu
@pytest.mark.parametrize("level", (10, 30))
def test_device_batch_blocks_above_4mib_exact_stride(L, level):
    """Three blocks of 4 MiB + 1 (33 sub-blocks, the last of one byte), at the minimum stride and with a pad."""
    if not L.LizardGPU_levelSupported(level):
        pytest.skip("level %d is not on the GPU path" % level)
    run_device_case(L, level, HUGE, 3, HUGE, 0, 3, range(3))
    run_device_case(L, level, HUGE, 3, 1, 61, 1, range(3))


# ---------------------------------------------------------------- host entries at their exact capacity ---------------------------

HOST_NB, HOST_BS, HOST_MARGIN = 67, 65537, 64


@pytest.mark.gpu
@pytest.mark.parametrize("level", (10, 30))
def test_host_batch_exact_stride(L, level):
    """LizardGPU_compressBlocks_host with dstStride == bound(blockSize) into a buffer with 64-byte canary margins."""
    src, what = make_source(HOST_NB, HOST_BS, HOST_BS - 1)
    stride = bound(HOST_BS)
    buf = np.full(HOST_MARGIN + HOST_NB * stride + HOST_MARGIN, CANARY, dtype=np.uint8)
    words = np.full(HOST_NB + 2, SENTINEL, dtype=np.uint32)
    before = src.copy()
    rc = L.LizardGPU_compressBlocks_host(src.ctypes.data, HOST_NB, HOST_BS, HOST_BS - 1, buf.ctypes.data + HOST_MARGIN, stride, words.ctypes.data + 4, level)
    assert rc == 0, L.LizardGPU_lastError()
    assert (buf[:HOST_MARGIN] == CANARY).all() and (buf[-HOST_MARGIN:] == CANARY).all()
    assert words[0] == SENTINEL and words[-1] == SENTINEL and (src == before).all()
    for i, (kind, variant, n) in enumerate(what):
        want = expected(kind, variant, n, level)
        assert words[1 + i] == len(want), (level, i, words[1 + i], len(want))
        assert (buf[HOST_MARGIN + i * stride:HOST_MARGIN + i * stride + len(want)] == want).all(), (level, i)


@pytest.mark.gpu
@pytest.mark.parametrize("level", (10, 30))
def test_host_packed_exact_capacity_and_one_byte_less(L, level):
    """dstCapacity exactly the sum of the oracle's sizes: offsets, sizes and bytes are the oracle's and nothing else is touched.
    One byte less: -LIZARDGPU_ERR_ARG, and nothing written behind the capacity."""
    src, what = make_source(HOST_NB, HOST_BS, HOST_BS - 1)
    want = [expected(kind, variant, n, level) for kind, variant, n in what]
    total = sum(len(w) for w in want)
    want_offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    for cap in (total, total - 1):
        buf = np.full(HOST_MARGIN + total + HOST_MARGIN, CANARY, dtype=np.uint8)
        offsets = np.full(HOST_NB + 3, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        words = np.full(HOST_NB + 2, SENTINEL, dtype=np.uint32)
        rc = L.LizardGPU_compressBlocks_host_packed(src.ctypes.data, HOST_NB, HOST_BS, HOST_BS - 1, buf.ctypes.data + HOST_MARGIN, cap,
                                                    offsets.ctypes.data + 8, words.ctypes.data + 4, level)
        assert (buf[:HOST_MARGIN] == CANARY).all(), (level, cap)
        assert (buf[HOST_MARGIN + cap:] == CANARY).all(), (level, cap, "written behind the capacity")
        assert offsets[0] == 0xA5A5A5A5A5A5A5A5 and offsets[-1] == 0xA5A5A5A5A5A5A5A5 and words[0] == SENTINEL and words[-1] == SENTINEL
        if cap == total:
            assert rc == 0, L.LizardGPU_lastError()
            assert (offsets[1:-1] == want_offsets).all() and (words[1:-1] == [len(w) for w in want]).all()
            assert (buf[HOST_MARGIN:HOST_MARGIN + total] == np.concatenate(want)).all()
        else:
            assert rc == -3, (rc, L.LizardGPU_lastError())       # -LIZARDGPU_ERR_ARG
