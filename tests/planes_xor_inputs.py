"""Where the bases of the batches of tests/planes_inputs.py / tests/bitplanes_inputs.py lie, for tests/test_planes_xor_emul.py (CPU SIMT
emulator) and tests/test_planes_xor_gpu.py (LizardGPU_splitPlanesXor_device / LizardGPU_joinPlanesXor_device).  No test in here."""


def base_offsets(cases, offsets):
    """Per buffer the offset of its base from a 16-byte boundary, or None for a buffer without a base (about every fifth).  The
    offset walks through OFFSETS relative to the src's, so that it equals the src's for a fifth of the buffers only."""
    return [None if i % 5 == 2 else offsets[(offsets.index(c[2]) + i // 5) % 5] for i, c in enumerate(cases)]


def place_bases(cases, b_off):
    """Where each base lies in the base arena (first byte 16-byte aligned); None where there is none."""
    pos, at = 0, []
    for (E, size, _, _), bo in zip(cases, b_off):
        if bo is None:
            at.append(None)
            continue
        pos += (-pos) % 16 + bo
        at.append(pos)
        pos += size
    return at, pos + 16
