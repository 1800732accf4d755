"""The batch of buffers that tests/test_planes_emul.py (CPU SIMT emulator) and tests/test_planes_gpu.py (LizardGPU_splitPlanes_device /
LizardGPU_joinPlanes_device) both move, its placement in two arenas, and the numpy model of the layout.  No test in here."""
import numpy as np

TILE = 16384                                                     # LZP_TILE_BYTES of lizard_amd/csrc/planes_kernels.h (the emulator test pins it)
ELEMS = (1, 2, 4, 8)
OFFSETS = (0, 1, 3, 8, 15)                                       # of src and of dst from a 16-byte boundary
GUARD = 64
FILL = 0x5A


def sizes_for(E):
    """Every size at which the kernels take another path: nothing, less than an element, the ragged end of a plane with and without
    whole 16-element groups in front of it, one wave step, one tile, more than one tile."""
    s = [0, 1, E - 1, E, E + 1, 15, 16, 17, 16 * E - 1, 16 * E, 16 * E + 1, 64 * 16 * E - 1, 64 * 16 * E, 64 * 16 * E + 1,
         TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
    return sorted(set(s))


def batch():
    """[(E, size, src offset, dst offset)]: every element size with every size; a size of up to 4 KiB under every pair of offsets, a
    larger one under five pairs that hold every offset on either side (the data stays small); plus 300 buffers of one byte (more
    table entries than a wave has lanes, tiles of one byte)."""
    out = []
    for E in ELEMS:
        for k, size in enumerate(sizes_for(E)):
            pairs = [(so, do) for so in OFFSETS for do in OFFSETS] if size <= 4097 else [(OFFSETS[i], OFFSETS[(i + k) % 5]) for i in range(5)]
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


def split_model(a, E):
    n = a.size // E
    return np.concatenate([a[:n * E].reshape(n, E).T.reshape(-1), a[n * E:]])


def join_model(a, E):
    n = a.size // E
    return np.concatenate([a[:n * E].reshape(E, n).T.reshape(-1), a[n * E:]])


def source(total, seed=5):
    return np.random.RandomState(seed).randint(0, 256, total, dtype=np.uint8)


def tiles_of(E, size):
    return 0 if not size else 1 if size < E else (size // E * E + TILE - 1) // TILE
