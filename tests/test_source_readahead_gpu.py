"""GPU: the blocks of tests/source_readahead_inputs.py at level 10 — the only level whose producers read the source ahead
(lizard_amd/csrc/lz_touch.h; the level-30 kernel keeps its loop) — sizes and bytes against the oracle: every size and kind as a
uniform launch of 64 blocks, the ragged batch at odd addresses as one batch of frames, and one launch of 2 080 blocks of
131 072 + 9 000 bytes in which every producer's cursor starts anew some twenty times."""
import numpy as np
import pytest

import source_readahead_inputs as inputs
import util
from test_producer_round_gpu import _device_batch

pytestmark = pytest.mark.gpu


def test_every_size_and_kind_in_launches_of_64_blocks():
    for name, data, _ in inputs.all_blocks():
        outs = _device_batch(data * 64, len(data), inputs.LEVEL)
        want = inputs.expected(data)
        assert len(outs) == 64
        assert all(o == want for o in outs), (name, [i for i, o in enumerate(outs) if o != want][:4])


def test_ragged_batch_at_odd_addresses():
    """One frame per block (128 KiB frame blocks: the block of 131 072 + 13 bytes is two), sources at odd addresses inside one tensor whose
    last byte is the last block's; every frame is the frame format around the oracle's blocks."""
    import torch
    from lizard_amd import api
    area, blocks = inputs.ragged_area()
    src = torch.from_numpy(np.frombuffer(area, dtype=np.uint8).copy()).cuda()
    frames = api.compress_frames_device([src[o:o + n] for o, n in blocks], inputs.LEVEL, block_size_id=1)
    torch.cuda.synchronize()
    for (o, n), f in zip(blocks, frames):
        assert src[o:o + n].data_ptr() % 2 == 1
        want = util.compose_frame(area[o:o + n], inputs.LEVEL, 1, 0, 0, util.oracle_compress)
        assert f.cpu().numpy().tobytes() == want, (o, n)


def test_2080_blocks_of_two_sub_blocks():
    """Ten different blocks, each 208 times: every producer goes through many blocks, with the cursor of the one before left wherever it
    stood — one that ends in the 515-byte-period block's long match included."""
    n = inputs.REPEAT_SIZE
    kinds = [util.datagen(n, 0.5, 0.0, 900 + s) for s in range(8)] + [inputs.incompressible(n), inputs.repeat515()]
    want = [inputs.expected(k) for k in kinds]
    outs = _device_batch(b"".join(kinds[i % 10] for i in range(2080)), n, inputs.LEVEL)
    assert len(outs) == 2080
    bad = [i for i, o in enumerate(outs) if o != want[i % 10]]
    assert not bad, bad[:8]
