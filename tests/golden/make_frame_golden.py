"""Writes tests/golden/frame_ref_linked.liz and frame_ref_independent.liz: frames made by the compiled reference
(oracle/_ref, LizardF_compressFrame) from golden_frame_input() — ten blocks of 128 KiB (more than one 1 MiB chunk of the frame decoder), content checksum and content size in
the header, well under 64 KiB each.  The linked one is the kind of frame this library never writes: its blocks copy from the
blocks before them.  Run from the repository root where oracle/_ref exists:  python tests/golden/make_frame_golden.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import util


def golden_frame_input():
    """9 * 128 KiB + 1000 bytes of very compressible generator output, the same 20 000 bytes coming round again and again (so
    that the blocks of a linked frame lean on the blocks before them)."""
    unit = util.datagen(20000, 0.9, 0.0, 77)
    return (unit * 60)[:9 * 131072 + 1000]


if __name__ == "__main__":
    data = golden_frame_input()
    for name, mode in (("frame_ref_linked.liz", 0), ("frame_ref_independent.liz", 1)):
        frame = util.reference_frame(data, util.frame_prefs(17, 1, 1, len(data), mode))
        assert frame is not None, "oracle/_ref is missing"
        assert len(frame) <= 65536
        open(os.path.join(HERE, name), "wb").write(frame)
        print(name, len(frame))
