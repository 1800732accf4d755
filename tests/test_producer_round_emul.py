"""CPU: the producer / consumer form of levels 10 / 30 (lizard_amd/csrc/lz_split.h) on the SIMT emulator, byte for byte against the
oracle, on small blocks chosen to walk every path of the producers' parse loop (tests/producer_round_inputs.py)."""
import ctypes

import pytest

import producer_round_inputs as inputs
import util


def emul_split(data, bs, level, nprod=2, ncons=1, seed=1):
    emu = util.emulator()
    emu.emul_compress_split.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    nb = (len(data) + bs - 1) // bs
    last = len(data) - (nb - 1) * bs
    stride = util.oracle().lzo_compress_bound(bs) + 64
    dst = ctypes.create_string_buffer(nb * stride)
    sizes = (ctypes.c_uint * nb)()
    src = ctypes.create_string_buffer(bytes(data), len(data))
    assert emu.emul_compress_split(src, nb, bs, last, dst, stride, sizes, level, nprod, ncons, seed) == 0
    return [dst.raw[i * stride:i * stride + sizes[i]] for i in range(nb)]


def test_oracle_compresses_what_is_meant_to_compress():
    """The cases that are there for their matches must not end as raw blocks in the oracle itself (a raw block hides the parse);
    the others are parsed and then stored raw."""
    for level in inputs.LEVELS:
        want = inputs.expected(level)
        for name, data, compressible in inputs.all_blocks():
            raw = len(data) + 1 + 4 * ((len(data) + 131071) // 131072)     # level byte + a 4-byte header per stored sub-block
            if compressible is None:
                continue
            if compressible:
                assert len(want[name]) < len(data), (level, name)
            else:
                assert len(want[name]) == raw, (level, name)


@pytest.mark.parametrize("level", inputs.LEVELS)
@pytest.mark.parametrize("size", inputs.GEN_SIZES)
def test_generated_blocks(level, size):
    """datagen P50, seeds 0-7, as one batch of eight blocks over two producers."""
    blocks = inputs.generated(size)
    outs = emul_split(b"".join(blocks), size, level, nprod=2, ncons=1, seed=size)
    want = inputs.expected(level)
    for seed, o in enumerate(outs):
        assert o == want["gen%d_s%d" % (size, seed)], (level, size, seed)


@pytest.mark.parametrize("level", inputs.LEVELS)
@pytest.mark.parametrize("case", range(len(inputs.special())))
def test_special_blocks(level, case):
    name, data, _ = inputs.special()[case]
    outs = emul_split(data, len(data), level, nprod=1, ncons=1, seed=case + 1)
    assert outs == [inputs.expected(level)[name]], (level, name)
