"""The batch of buffers that tests/test_bitplanes_emul.py (CPU SIMT emulator) and tests/test_bitplanes_gpu.py
(LizardGPU_splitBitPlanes_device / LizardGPU_joinBitPlanes_device) both move, its placement in two arenas, and the numpy model of the
bit-plane layout (include/lizard_amd.h Part 3c).  No test in here."""
import numpy as np

TILE = 16384                                                     # LZP_TILE_BYTES of lizard_amd/csrc/planes_kernels.h (the emulator test pins it)
STEP = 2048                                                      # LZB_STEP_ELEMS of lizard_amd/csrc/bitplanes_kernels.h: elements of a wave step
ELEMS = (1, 2, 4, 8)
OFFSETS = (0, 1, 3, 8, 15)                                       # of src and of dst from a 16-byte boundary
GUARD = 64
FILL = 0x5A


def sizes_for(E):
    """Every size at which the kernels take another path: nothing, less than an element, fewer than 8 elements (no plane byte), the
    ragged end of the planes (whole groups of 8 elements that fill no quad of 128) with and without whole quads in front of it,
    a lane's 32 elements, one wave step, one tile, more than one tile, and — beyond one tile — a size whose last tile holds whole
    quads, a ragged end, n % 8 elements that are copied and bytes behind the last whole element."""
    s = [0, 1, E - 1, E, 8 * E - 1, 8 * E, 8 * E + 1, 32 * E - 1, 32 * E + 1, 128 * E - 1, 128 * E, 128 * E + 1,
         STEP * E - 1, STEP * E, STEP * E + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5,
         TILE + (3 * 128 + 5 * 8 + 3) * E + E // 2]
    return sorted(set(s))


def batch():
    """[(E, size, src offset, dst offset)]: every element size with every size; a size of up to 4 KiB under every pair of offsets, a
    larger one under five pairs that hold every offset on either side (the data stays small); plus 300 buffers of one byte (more
    table entries than a wave has lanes, tiles of one byte)."""
    out = []
    for E in ELEMS:
        for k, size in enumerate(sizes_for(E)):
            pairs = [(so, do) for so in OFFSETS for do in OFFSETS] if size <= 4096 else [(OFFSETS[i], OFFSETS[(i + k) % 5]) for i in range(5)]
            out += [(E, size, so, do) for so, do in pairs]
    out += [(ELEMS[i % 4], 1, OFFSETS[i % 5], OFFSETS[(i // 5) % 5]) for i in range(300)]
    return out


def place(cases, base=0):
    """Where each buffer lies in the src arena and in the dst arena, whose first bytes are at addresses congruent to `base` mod 16:
    (src positions, dst positions, src arena bytes, dst arena bytes).  Every dst has GUARD bytes in front of it and behind it that
    belong to no buffer."""
    def up16(x):
        return x + (-(x + base)) % 16
    sp, dp, s_at, d_at = 0, GUARD, [], []
    for E, size, so, do in cases:
        sp = up16(sp) + so
        s_at.append(sp)
        sp += size
        dp = up16(dp) + do
        d_at.append(dp)
        dp += size + GUARD
    return s_at, d_at, sp + 16, dp + 16


def bits_split_model(a, E):
    n = a.size // E
    n8 = n - n % 8
    bits = np.unpackbits(a[:n8 * E].reshape(n8, E), axis=1, bitorder="little")
    planes = np.packbits(np.ascontiguousarray(bits.T), axis=1, bitorder="little")
    return np.concatenate([planes.reshape(-1), a[n8 * E:]])


def bits_join_model(b, E):
    n = b.size // E
    n8 = n - n % 8
    bits = np.unpackbits(b[:n8 * E].reshape(8 * E, n8 // 8), axis=1, bitorder="little")
    return np.concatenate([np.packbits(np.ascontiguousarray(bits.T), axis=1, bitorder="little").reshape(-1), b[n8 * E:]])


def source(total, seed=5):
    return np.random.RandomState(seed).randint(0, 256, total, dtype=np.uint8)


def tiles_of(E, size):
    return 0 if not size else 1 if size < E else (size // E * E + TILE - 1) // TILE
