"""Host-side mirror of the reference's block-compression interface (inikep/lizard lib/lizard_compress.h)
plus the batch entry points the GPU needs. Names, argument meaning and error behaviour follow the
reference: sizes in bytes, `Lizard_compress` returns b"" on failure where the C function returns 0.

PyTorch appears only as the owner of device memory and streams (plumbing); all compute is in
liblizard_amd.so.
"""
import ctypes

import numpy as np

from . import _lib

LIZARD_MIN_CLEVEL = 10
LIZARD_MAX_CLEVEL = 49
LIZARD_DEFAULT_CLEVEL = 17
LIZARD_MAX_INPUT_SIZE = 0x7E000000
LIZARD_BLOCK_SIZE = 1 << 17


def Lizard_compressBound(isize):
    """reference lib/lizard_compress.h:124 (LIZARD_COMPRESSBOUND)."""
    if isize < 0 or isize > LIZARD_MAX_INPUT_SIZE:
        return 0
    return isize + 1 + 1 + ((isize // LIZARD_BLOCK_SIZE) + 1) * 4


def Lizard_compress(src, compressionLevel=LIZARD_MIN_CLEVEL, maxDstSize=None):
    """reference lib/lizard_compress.c:596 — one block through the GPU path. Returns the compressed bytes,
    or b"" when the C function returns 0 (does not fit in maxDstSize / level not on the GPU path)."""
    L = _lib.lib()
    src = bytes(src)
    if maxDstSize is None:
        maxDstSize = Lizard_compressBound(len(src))
    dst = ctypes.create_string_buffer(max(maxDstSize, 1))
    n = L.Lizard_compress(src, dst, len(src), maxDstSize, compressionLevel)
    return dst.raw[:n]


def level_supported(level):
    return bool(_lib.lib().LizardGPU_levelSupported(level))


def compress_blocks(data, block_size, level=LIZARD_MIN_CLEVEL):
    """Split host `data` into independent blocks of block_size (last one ragged) and compress them in one
    batched GPU call. Returns a list of bytes, block i == Lizard_compress_extState(zero state, block i)."""
    L = _lib.lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    n = buf.size
    if n == 0:
        return []
    nb = (n + block_size - 1) // block_size
    last = n - (nb - 1) * block_size
    stride = Lizard_compressBound(block_size)
    out = np.empty(nb * stride, dtype=np.uint8)
    sizes = np.zeros(nb, dtype=np.uint32)
    rc = L.LizardGPU_compressBlocks_host(buf.ctypes.data, nb, block_size, last, out.ctypes.data, stride,
                                         sizes.ctypes.data, level)
    _lib.check(rc, "LizardGPU_compressBlocks_host")
    return [out[i * stride:i * stride + int(sizes[i])].tobytes() for i in range(nb)]


def compress_blocks_device(src, block_size, level=LIZARD_MIN_CLEVEL, dst=None, sizes=None, n_bytes=None):
    """Device-resident batch: `src` is a torch uint8 CUDA tensor holding the blocks back to back.
    Enqueues on torch's current stream and returns (dst, sizes, stride): dst is a uint8 tensor of
    nb*stride bytes (slot i at i*stride), sizes an int32 tensor view of the uint32 sizes."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    n = int(src.numel()) if n_bytes is None else int(n_bytes)
    nb = (n + block_size - 1) // block_size
    last = n - (nb - 1) * block_size
    stride = (Lizard_compressBound(block_size) + 63) & ~63
    if dst is None:
        dst = torch.empty(nb * stride, dtype=torch.uint8, device=src.device)
    if sizes is None:
        sizes = torch.zeros(nb, dtype=torch.int32, device=src.device)
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = torch.cuda.current_stream(src.device).cuda_stream
    rc = L.LizardGPU_compressBlocks_device(src.data_ptr(), nb, block_size, last, dst.data_ptr(), stride,
                                           sizes.data_ptr(), level, ctypes.c_void_p(stream))
    _lib.check(rc, "LizardGPU_compressBlocks_device")
    return dst, sizes, stride


def _host_array(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)


def decompress_blocks(blocks, max_block_size):
    """Decode independent compressed blocks (what compress_blocks returns) in one batched GPU call; every block decodes to at
    most max_block_size bytes. Returns a list of bytes; a corrupt block raises."""
    L = _lib.lib()
    blocks = [bytes(b) for b in blocks]
    nb = len(blocks)
    if nb == 0:
        return []
    offsets = np.zeros(nb + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(b) for b in blocks], dtype=np.uint64)
    src = np.frombuffer(b"".join(blocks) or b"\0", dtype=np.uint8)
    out = np.empty(nb * max_block_size, dtype=np.uint8)
    sizes = np.zeros(nb, dtype=np.uint32)
    rc = L.LizardGPU_decompressBlocks_host(src.ctypes.data, offsets.ctypes.data, nb, out.ctypes.data, max_block_size,
                                           sizes.ctypes.data)
    _lib.check(rc, "LizardGPU_decompressBlocks_host")
    bad = [i for i in range(nb) if int(sizes[i]) == 0xFFFFFFFF]
    if bad:
        raise _lib.LizardAmdError(f"decompress_blocks: block {bad[0]} is corrupt or does not fit {max_block_size} bytes")
    return [out[i * max_block_size:i * max_block_size + int(sizes[i])].tobytes() for i in range(nb)]


def decompress_blocks_device(src, sizes, stride, block_size, dst=None, out_sizes=None):
    """Device-resident batch in the layout compress_blocks_device returns: block i is sizes[i] bytes at src + i*stride.
    Enqueues on torch's current stream and returns (dst, out_sizes): block i decoded at dst + i*block_size, out_sizes[i] its
    size as int32 (-1: corrupt or larger than block_size)."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    assert sizes.is_cuda and sizes.dtype == torch.int32 and sizes.is_contiguous()
    nb = int(sizes.numel())
    if dst is None:
        dst = torch.empty(nb * block_size, dtype=torch.uint8, device=src.device)
    if out_sizes is None:
        out_sizes = torch.zeros(nb, dtype=torch.int32, device=src.device)
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = torch.cuda.current_stream(src.device).cuda_stream
    rc = L.LizardGPU_decompressBlocks_device(src.data_ptr(), stride, sizes.data_ptr(), nb, dst.data_ptr(), block_size,
                                             out_sizes.data_ptr(), ctypes.c_void_p(stream))
    _lib.check(rc, "LizardGPU_decompressBlocks_device")
    return dst, out_sizes


class _FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_uint), ("blockMode", ctypes.c_uint), ("contentChecksumFlag", ctypes.c_uint),
                ("frameType", ctypes.c_uint), ("contentSize", ctypes.c_ulonglong), ("reserved", ctypes.c_uint * 2)]


class _FramePrefs(ctypes.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", ctypes.c_uint),
                ("reserved", ctypes.c_uint * 4)]


def compress_frame(data, level=LIZARD_MIN_CLEVEL, block_size_id=0, checksum=False, content_size=False, independent=True):
    """One Lizard frame (reference lib/lizard_frame.h) through LizardGPU_compressFrame: every block compressed in one batch
    on the GPU. Linked frames (independent=False) larger than one block are refused by that strict entry."""
    L = _lib.lib()
    buf = _host_array(data)
    p = _FramePrefs()
    p.frameInfo.blockSizeID = block_size_id
    p.frameInfo.blockMode = 1 if independent else 0
    p.frameInfo.contentChecksumFlag = 1 if checksum else 0
    p.frameInfo.contentSize = buf.size if content_size else 0
    p.compressionLevel = level
    cap = L.LizardGPU_compressFrameBound(buf.size, ctypes.byref(p))
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = _lib.check_frame(L.LizardGPU_compressFrame(out.ctypes.data, cap, buf.ctypes.data, buf.size, ctypes.byref(p)),
                         "LizardGPU_compressFrame")
    return out[:n].tobytes()


def compress_frame_device(src, level=LIZARD_MIN_CLEVEL, block_size_id=0, checksum=False, content_size=False, dst=None):
    """One Lizard frame for `src`, a contiguous uint8 CUDA tensor, written into a uint8 CUDA tensor on the same device
    (LizardGPU_compressFrame_device) on torch's current stream: the bytes LizardGPU_compressFrame writes for the same input.  No
    payload crosses PCIe unless `checksum` asks for the content checksum, which is computed on the host.  Without `dst` the
    output has LizardGPU_compressFrameBound bytes.  Returns (dst, n): the frame is dst[:n]; an error code raises."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    size = int(src.numel())
    p = _FramePrefs()
    p.frameInfo.blockSizeID = block_size_id
    p.frameInfo.blockMode = 1
    p.frameInfo.contentChecksumFlag = 1 if checksum else 0
    p.frameInfo.contentSize = size if content_size else 0
    p.compressionLevel = level
    if dst is None:
        cap = _lib.check_frame(L.LizardGPU_compressFrameBound(size, ctypes.byref(p)), "LizardGPU_compressFrameBound")
        dst = torch.empty(cap, dtype=torch.uint8, device=src.device)
    assert dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous() and dst.device == src.device
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    n = _lib.check_frame(L.LizardGPU_compressFrame_device(dst.data_ptr(), int(dst.numel()), src.data_ptr(), size, ctypes.byref(p), stream),
                         "LizardGPU_compressFrame_device")
    return dst, n


def compress_frames_device(tensors, level=LIZARD_MIN_CLEVEL, block_size_id=0, checksum=False, content_size=False):
    """One Lizard frame for each of `tensors`, a sequence of contiguous uint8 CUDA tensors on one device (zero-length ones allowed),
    in ONE call of LizardGPU_compressFrames_device on torch's current stream: frame i is the bytes compress_frame_device writes for
    tensor i.  No payload crosses PCIe, with or without `checksum`.  One output tensor holds every frame's
    LizardGPU_compressFrameBound-sized region at 256-byte-aligned offsets; returns the list of views region_i[:n_i].  A refused frame
    raises LizardAmdError naming the first such frame's index and error; so does a failure of the machinery."""
    return _compress_frames_device(tensors, level, block_size_id, checksum, content_size, 0)


def _compress_frames_device(tensors, level, block_size_id, checksum, content_size, slack):
    """compress_frames_device with `slack` bytes of room behind every frame's LizardGPU_compressFrameBound."""
    import torch
    L = _lib.lib()
    tensors = list(tensors)
    if not tensors:
        return []
    device = tensors[0].device
    for t in tensors:
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == device
    n = len(tensors)
    p = _FramePrefs()
    p.frameInfo.blockSizeID = block_size_id
    p.frameInfo.blockMode = 1
    p.frameInfo.contentChecksumFlag = 1 if checksum else 0
    p.frameInfo.contentSize = 1 if content_size else 0          # (non-zero: "write each frame's own size")
    p.compressionLevel = level
    sizes = (ctypes.c_size_t * n)(*[int(t.numel()) for t in tensors])
    caps = (ctypes.c_size_t * n)(*[_lib.check_frame(L.LizardGPU_compressFrameBound(s, ctypes.byref(p)), "LizardGPU_compressFrameBound") + slack for s in sizes])
    offsets, total = [], 0
    for cap in caps:
        offsets.append(total)
        total += (cap + 255) & ~255
    out = torch.empty(total, dtype=torch.uint8, device=device)
    srcs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    dsts = (ctypes.c_void_p * n)(*[out.data_ptr() + o for o in offsets])
    results = (ctypes.c_size_t * n)()
    L.LizardGPU_setDevice(device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(L.LizardGPU_compressFrames_device(n, dsts, caps, srcs, sizes, results, ctypes.byref(p), stream), "LizardGPU_compressFrames_device")
    for i, r in enumerate(results):
        if L.LizardGPU_frameIsError(r):
            raise _lib.LizardAmdError(f"LizardGPU_compressFrames_device: frame {i}: {L.LizardF_getErrorName(r).decode()}")
    return [out[o:o + int(r)] for o, r in zip(offsets, results)]


def frame_info(data):
    """Header fields and record table of the frame at the start of `data` (host code, no GPU): a dict with block_size_id,
    independent, checksum, skippable, content_size, n_records, frame_bytes, bound."""
    L = _lib.lib()
    buf = _host_array(data)
    info = _FrameInfo()
    n, fb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = L.LizardGPU_frameIndex(buf.ctypes.data, buf.size, ctypes.byref(info), None, None, 0, ctypes.byref(n), ctypes.byref(fb))
    if rc:
        _lib.check_frame((1 << 64) + rc, "LizardGPU_frameIndex")
    return {"block_size_id": info.blockSizeID, "independent": bool(info.blockMode), "checksum": bool(info.contentChecksumFlag),
            "skippable": bool(info.frameType), "content_size": info.contentSize, "n_records": n.value, "frame_bytes": fb.value,
            "bound": L.LizardGPU_decompressFrameBound(buf.ctypes.data, buf.size)}


def decompress_frame(data):
    """Decode the frame(s) in `data` on the GPU (LizardGPU_decompressFrame); concatenated frames are decoded one after the
    other and joined, skippable frames contribute nothing."""
    L = _lib.lib()
    buf = _host_array(data)
    out, pos = [], 0
    while pos < buf.size:
        src = buf[pos:]
        cap = _lib.check_frame(L.LizardGPU_decompressFrameBound(src.ctypes.data, src.size), "LizardGPU_decompressFrameBound")
        dst = np.empty(max(cap, 1), dtype=np.uint8)
        used = ctypes.c_size_t(0)
        n = _lib.check_frame(L.LizardGPU_decompressFrame(dst.ctypes.data, cap, src.ctypes.data, src.size, ctypes.byref(used)),
                             "LizardGPU_decompressFrame")
        out.append(dst[:n].tobytes())
        pos += used.value
    return b"".join(out)


FRAME_SKIP_CHECKSUM = 1
_INDEX_GUESS = 1 << 16          # records the first walk of frame_index_device has tables for (16 GiB of output at 256 KiB blocks)


def frame_index_device(src):
    """LizardGPU_frameIndex_device: header fields and record table of the frame at the start of `src`, a contiguous uint8 CUDA
    tensor, walked on the device on torch's current stream.  The keys of frame_info, plus "offsets" (int64) and "words" (int32
    view of the LE32 record words: negative = stored raw) as tensors on src's device."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    info = _FrameInfo()
    n, fb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    size = int(src.numel())
    room = min(_INDEX_GUESS, size // 5 + 1)                    # (a record is 5 bytes at least)
    while True:                                                # one walk, unless the frame has more records than the guess
        offsets = torch.empty(room, dtype=torch.int64, device=src.device)
        words = torch.empty(room, dtype=torch.int32, device=src.device)
        rc = L.LizardGPU_frameIndex_device(src.data_ptr(), size, ctypes.byref(info), offsets.data_ptr(), words.data_ptr(), room,
                                           ctypes.byref(n), ctypes.byref(fb), stream)
        if rc:
            _lib.check_frame((1 << 64) + rc, "LizardGPU_frameIndex_device")
        if n.value <= room:
            break
        room = n.value
    offsets, words = offsets[:n.value], words[:n.value]
    bound = 0
    if n.value:
        block = L.LizardGPU_frameBlockSize(info.blockSizeID)
        bound = int(torch.where(words < 0, words & 0x7FFFFFFF, torch.full_like(words, block)).sum(dtype=torch.int64).item())
        if info.contentSize and info.contentSize < bound:
            bound = int(info.contentSize)
    return {"block_size_id": info.blockSizeID, "independent": bool(info.blockMode), "checksum": bool(info.contentChecksumFlag),
            "skippable": bool(info.frameType), "content_size": info.contentSize, "n_records": n.value, "frame_bytes": fb.value,
            "bound": bound, "offsets": offsets, "words": words}


def decompress_frame_device(src, dst=None, verify_checksum=True):
    """Decode the frame(s) in `src`, a contiguous uint8 CUDA tensor, into a uint8 CUDA tensor on the same device
    (LizardGPU_decompressFrame_device) on torch's current stream: neither the frame nor the decoded bytes cross PCIe, unless
    verify_checksum asks for the content checksum, which is computed on the host.  Concatenated frames are decoded one after the
    other, skippable frames contribute nothing.  Without `dst` the output is sized by a walk of every frame (frame_index_device).
    Returns the decoded bytes (a view of `dst` when given); an error code raises."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    size = int(src.numel())
    if dst is None:
        total, pos = 0, 0
        while pos < size:
            info = frame_index_device(src[pos:])
            total += info["bound"]
            pos += info["frame_bytes"]
        dst = torch.empty(max(total, 1), dtype=torch.uint8, device=src.device)[:total]
    assert dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous() and dst.device == src.device
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    flags = 0 if verify_checksum else FRAME_SKIP_CHECKSUM
    cap, pos, out = int(dst.numel()), 0, 0
    while pos < size:
        used = ctypes.c_size_t(0)
        n = _lib.check_frame(L.LizardGPU_decompressFrame_device(dst.data_ptr() + out, cap - out, src.data_ptr() + pos, size - pos,
                                                                ctypes.byref(used), flags, stream), "LizardGPU_decompressFrame_device")
        out += n
        pos += used.value
    return dst[:out]


def _frame_ptrs(frames):
    import torch
    device = frames[0].device
    for t in frames:
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == device
    n = len(frames)
    return device, (ctypes.c_void_p * n)(*[t.data_ptr() for t in frames]), (ctypes.c_size_t * n)(*[int(t.numel()) for t in frames])


def frames_info_device(frames):
    """LizardGPU_framesInfo_device: the header fields and record counts of `frames`, a sequence of contiguous uint8 CUDA tensors on one
    device that hold one frame each, all walked on the device side by side in one launch on torch's current stream, with one host
    wait.  A list of dicts with the keys of frame_info except "bound" (and without the tables of frame_index_device).  A refused
    frame raises LizardAmdError naming the first such frame's index and error."""
    import torch
    L = _lib.lib()
    frames = list(frames)
    if not frames:
        return []
    device, srcs, sizes = _frame_ptrs(frames)
    n = len(frames)
    infos, nrec, fbytes, codes = (_FrameInfo * n)(), (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)(), (ctypes.c_int * n)()
    L.LizardGPU_setDevice(device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(L.LizardGPU_framesInfo_device(n, srcs, sizes, infos, nrec, fbytes, codes, stream), "LizardGPU_framesInfo_device")
    for i, rc in enumerate(codes):
        if rc:
            raise _lib.LizardAmdError(f"LizardGPU_framesInfo_device: frame {i}: {L.LizardF_getErrorName((1 << 64) + rc).decode()}")
    return [{"block_size_id": f.blockSizeID, "independent": bool(f.blockMode), "checksum": bool(f.contentChecksumFlag),
             "skippable": bool(f.frameType), "content_size": f.contentSize, "n_records": int(k), "frame_bytes": int(b)}
            for f, k, b in zip(infos, nrec, fbytes)]


def decompress_frames_device(frames, sizes=None, verify_checksum=True):
    """Decode `frames`, a sequence of contiguous uint8 CUDA tensors on one device that hold ONE frame each (what compress_frames_device
    returns), in ONE call of LizardGPU_decompressFrames_device on torch's current stream: neither the frames nor the decoded bytes
    cross PCIe, with or without verify_checksum — the content checksums are computed on the device.  One output tensor holds every
    frame's region at 256-byte-aligned offsets; returns the list of views region_i[:n_i].
    With `sizes`, the caller's known decoded sizes, region i has exactly sizes[i] bytes and no extra walk is made.  Without, one
    frames_info_device call sizes region i: the header's content size when it has one, else n_records times
    LizardGPU_frameBlockSize(block_size_id).  Both are upper bounds of the decoded size; the second is looser than
    LizardGPU_decompressFrameBound (it counts a stored-raw record as a whole block too), by less than one block per stored-raw record.
    Exact sizes cost nothing but one case: a frame whose last block is ONE byte is decoded by the single-frame entry when its region
    has no room to spare (that block's record is longer than the byte it decodes to); the answer is the same.
    A refused frame raises LizardAmdError naming the first such frame's index and error; so does a tensor with bytes behind its frame,
    and a failure of the machinery."""
    import torch
    L = _lib.lib()
    frames = list(frames)
    if not frames:
        return []
    device, srcs, src_sizes = _frame_ptrs(frames)
    n = len(frames)
    if sizes is None:
        infos = frames_info_device(frames)
        sizes = [0 if f["skippable"] else f["content_size"] or f["n_records"] * L.LizardGPU_frameBlockSize(f["block_size_id"]) for f in infos]
    sizes = [int(s) for s in sizes]
    assert len(sizes) == n
    offsets, total = [], 0
    for cap in sizes:
        offsets.append(total)
        total += (cap + 255) & ~255
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    dsts = (ctypes.c_void_p * n)(*[out.data_ptr() + o for o in offsets])
    results, used = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    L.LizardGPU_setDevice(device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    flags = 0 if verify_checksum else FRAME_SKIP_CHECKSUM
    _lib.check(L.LizardGPU_decompressFrames_device(n, dsts, (ctypes.c_size_t * n)(*sizes), srcs, src_sizes, results, used, flags, stream),
               "LizardGPU_decompressFrames_device")
    for i, r in enumerate(results):
        if L.LizardGPU_frameIsError(r):
            raise _lib.LizardAmdError(f"LizardGPU_decompressFrames_device: frame {i}: {L.LizardF_getErrorName(r).decode()}")
        if used[i] < src_sizes[i]:
            raise _lib.LizardAmdError(f"LizardGPU_decompressFrames_device: frame {i}: {src_sizes[i] - used[i]} bytes behind the frame's end")
    return [out[o:o + int(r)] for o, r in zip(offsets, results)]


STREAM_FRAME_SLACK = 8          # bytes compress_stream_device gives every frame beyond LizardGPU_compressFrameBound (5 are needed)


def compress_stream_device_into(tensors, dst=None, prefixes=None, level=LIZARD_MIN_CLEVEL, block_size_id=0, checksum=False, content_size=True,
                                seekable=False):
    """A .liz STREAM for `tensors` — contiguous uint8 CUDA tensors on one device, zero-length ones allowed — written into ONE uint8 CUDA
    tensor in ONE call of LizardGPU_compressStream_device on torch's current stream: per tensor `prefixes[i]` (host bytes, opaque to
    the entry; None: no prefixes) and then the frame compress_frame_device writes for tensor i with 8 bytes more than its
    LizardGPU_compressFrameBound.  Where frame i starts is decided on the device, so every compressed byte is written once, to its
    place, and no payload byte crosses PCIe, with or without `checksum`.  Without `dst` the output has
    LizardGPU_compressStreamBound bytes — the only allocation of the call; a `dst` that is too small raises (dstMaxSize_tooSmall),
    as does a tensor the single-frame entry would refuse, naming the first such tensor.  Returns (dst[:n], offsets): the stream, and
    the n + 1 places where prefix 0, prefix 1, ... start and the stream ends.
    seekable=True (opt-in; without it the call is what it was): LizardGPU_compressSeekableStream_device — the same bytes, and behind
    them a seek table (a skippable frame, include/lizard_amd.h Part 3b) written by one more kernel of the same call; offsets[n] is
    then where the TABLE starts, and `dst` needs LizardGPU_seekTableBytes(n) bytes more."""
    import torch
    L = _lib.lib()
    tensors = list(tensors)
    if not tensors:
        raise ValueError("compress_stream_device_into: no tensors")
    device = tensors[0].device
    for t in tensors:
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.device == device
    n = len(tensors)
    p = _FramePrefs()
    p.frameInfo.blockSizeID = block_size_id
    p.frameInfo.blockMode = 1
    p.frameInfo.contentChecksumFlag = 1 if checksum else 0
    p.frameInfo.contentSize = 1 if content_size else 0          # (non-zero: "write each frame's own size")
    p.compressionLevel = level
    sizes = (ctypes.c_size_t * n)(*[int(t.numel()) for t in tensors])
    srcs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    pre_ptrs = pre_sizes = blob = None
    if prefixes is not None:
        prefixes = [bytes(x) for x in prefixes]
        assert len(prefixes) == n
        blob = np.frombuffer(b"".join(prefixes) + b"\0", dtype=np.uint8)    # (kept alive until the call returns)
        pre_sizes = (ctypes.c_size_t * n)(*[len(x) for x in prefixes])
        at, ptrs = 0, []
        for x in prefixes:
            ptrs.append(blob.ctypes.data + at)
            at += len(x)
        pre_ptrs = (ctypes.c_void_p * n)(*ptrs)
    if dst is None:
        cap = _lib.check_frame(L.LizardGPU_compressStreamBound(n, sizes, pre_sizes, ctypes.byref(p)), "LizardGPU_compressStreamBound")
        if seekable:
            cap += _lib.check_frame(L.LizardGPU_seekTableBytes(n), "LizardGPU_seekTableBytes")
        dst = torch.empty(cap, dtype=torch.uint8, device=device)
    assert dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous() and dst.device == device
    offsets = (ctypes.c_uint64 * (n + 1))()
    failed = ctypes.c_size_t(0)
    L.LizardGPU_setDevice(device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    name = "LizardGPU_compressSeekableStream_device" if seekable else "LizardGPU_compressStream_device"
    r = getattr(L, name)(dst.data_ptr(), int(dst.numel()), n, srcs, sizes, pre_ptrs, pre_sizes, ctypes.byref(p), offsets, ctypes.byref(failed), stream)
    if L.LizardGPU_frameIsError(r):
        raise _lib.LizardAmdError(f"{name}: {L.LizardF_getErrorName(r).decode()} "
                                  f"{L.LizardGPU_lastError().decode(errors='replace')}".strip())
    return dst[:r], [int(o) for o in offsets]


def _compress_stream_device_cat(tensors, level=LIZARD_MIN_CLEVEL, block_size_id=0, checksum=False):
    """compress_stream_device as it was before LizardGPU_compressStream_device: compress_frames_device(..., content_size=True) with
    STREAM_FRAME_SLACK bytes of room behind every frame's bound, and one torch.cat of the frame views.  Kept as the yardstick of the
    tests and of scripts/stream_compress_device_bench.py: the same bytes, every one of them written twice."""
    import torch
    frames = _compress_frames_device(tensors, level, block_size_id, checksum, True, STREAM_FRAME_SLACK)
    if not frames:
        raise ValueError("compress_stream_device: no tensors")
    return torch.cat(frames)


def compress_stream_device(tensors, level=LIZARD_MIN_CLEVEL, block_size_id=0, checksum=False, seekable=False):
    """A .liz STREAM for `tensors`: one frame with content size per tensor, back to back, in ONE call of
    LizardGPU_compressStream_device (compress_stream_device_into without prefixes) into ONE allocation of
    LizardGPU_compressStreamBound bytes.  Returns one uint8 CUDA tensor, a view of that allocation: the frames, which the
    reference's decoder reads frame after frame and decompress_stream_device decodes in ONE batch, because every header says how
    many bytes its frame decodes to.
    Every frame gets STREAM_FRAME_SLACK = 8 bytes of room more than LizardGPU_compressFrameBound (see the note at that function in
    include/lizard_amd.h; the stream bound counts them): a block of ONE byte makes a record with 6 bytes of payload,
    5 more than the bound counts.  The 8 bytes a header without content size leaves unused hide that; a 15-byte header does not, so
    with the bound alone a tensor of one byte — or one whose size is one more than a multiple of the block size — is refused.
    seekable=True: the same frames with a seek table behind them (compress_stream_device_into), which decompress_stream_device(seek=True)
    decodes without the serial walk over the frames."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("compress_stream_device: no tensors")
    return compress_stream_device_into(tensors, None, None, level, block_size_id, checksum, True, seekable)[0]


class _SeekEntry(ctypes.Structure):
    """LizardGPU_seekEntry_t"""
    _fields_ = [("offset", ctypes.c_uint64), ("decodedBytes", ctypes.c_uint64), ("prefixBytes", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


SEEK_USABLE, SEEK_NONE, SEEK_MORE, SEEK_DAMAGED = 0, 1, 2, 3      # LIZARDGPU_SEEK_*


def stream_seek_table_device(src):
    """LizardGPU_seekTable_device: the seek table at the end of the stream in `src`, a contiguous uint8 CUDA tensor — two small copies
    from its last bytes on torch's current stream, no walk.  One dict per item of the writing call: "offset" (where its prefix starts),
    "prefix_bytes", "frame_bytes" (of the frame behind the prefix) and "decoded_bytes"; or None when the stream has no usable table
    (none at all, or a damaged one: the stream's frames decode as ever)."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    room = 1024
    while True:
        entries, n, at = (_SeekEntry * room)(), ctypes.c_size_t(0), ctypes.c_uint64(0)
        rc = _lib.check(L.LizardGPU_seekTable_device(src.data_ptr(), int(src.numel()), entries, room, ctypes.byref(n), ctypes.byref(at), stream),
                        "LizardGPU_seekTable_device")
        if rc != SEEK_USABLE:
            return None
        if n.value <= room:
            break
        room = n.value
    ends = [int(e.offset) for e in entries[1:n.value]] + [int(at.value)]
    return [{"offset": int(e.offset), "prefix_bytes": int(e.prefixBytes), "frame_bytes": end - int(e.offset) - int(e.prefixBytes),
             "decoded_bytes": int(e.decodedBytes)} for e, end in zip(entries[:n.value], ends)]


def stream_info_device(src):
    """LizardGPU_streamIndex_device: the frames of the stream in `src`, a contiguous uint8 CUDA tensor that holds frames back to back,
    found by one wave that follows the chain of frames on the device on torch's current stream.  A list with one dict per frame: the
    keys frames_info_device returns, plus "offset", the frame's place in `src`.  A refused frame raises LizardAmdError naming its
    index and offset."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    size = int(src.numel())
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    room = min(max(size // 8, 1), 1 << 16)                     # (no frame is shorter than 8 bytes)
    while True:                                                # one walk, unless the stream has more frames than the guess
        offs, fbytes = (ctypes.c_uint64 * room)(), (ctypes.c_uint64 * room)()
        infos, nrec = (_FrameInfo * room)(), (ctypes.c_size_t * room)()
        n, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = L.LizardGPU_streamIndex_device(src.data_ptr(), size, offs, fbytes, infos, nrec, room, ctypes.byref(n), ctypes.byref(total), stream)
        if rc:
            raise _lib.LizardAmdError(f"LizardGPU_streamIndex_device: frame {n.value} at offset {total.value}: "
                                      f"{L.LizardF_getErrorName((1 << 64) + rc).decode()} ({L.LizardGPU_lastError().decode()})")
        if n.value <= room:
            break
        room = n.value
    return [{"block_size_id": f.blockSizeID, "independent": bool(f.blockMode), "checksum": bool(f.contentChecksumFlag),
             "skippable": bool(f.frameType), "content_size": f.contentSize, "n_records": int(k), "frame_bytes": int(b), "offset": int(o)}
            for f, k, b, o in zip(infos[:n.value], nrec[:n.value], fbytes[:n.value], offs[:n.value])]


def decompress_stream_device(src, dst=None, size=None, verify_checksum=True, seek=False):
    """Decode the stream of frames in `src`, a contiguous uint8 CUDA tensor, into one uint8 CUDA tensor on the same device
    (LizardGPU_decompressStream_device) on torch's current stream: the frames are found on the device and decoded in batches, a stream
    whose frames carry their content size (compress_stream_device) in ONE batch; neither the frames nor the decoded bytes cross PCIe.
    Without `dst` the output has `size` bytes, or, without `size`, what one stream_info_device call promises: per frame the content
    size, else n_records times the frame's block size (an upper bound).  Returns (dst_view, n_frames): the decoded bytes of all
    frames joined, and how many frames there were.  An error code raises LizardAmdError naming the offset of the refused frame.
    seek=True: LizardGPU_decompressSeekableStream_device — the same answer for every stream; one that ends in a usable seek table
    (compress_stream_device(..., seekable=True)) is decoded from the table's places in one batch without the walk, and without
    `dst` and `size` the table gives the size; any other stream takes the path above."""
    import torch
    L = _lib.lib()
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    if dst is None:
        if size is None and seek:
            table = stream_seek_table_device(src)
            size = None if table is None else sum(e["decoded_bytes"] for e in table)
        if size is None:
            size = sum(0 if f["skippable"] else f["content_size"] or f["n_records"] * L.LizardGPU_frameBlockSize(f["block_size_id"])
                       for f in stream_info_device(src))
        dst = torch.empty(max(int(size), 1), dtype=torch.uint8, device=src.device)[:int(size)]
    assert dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous() and dst.device == src.device
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    used, frames, decoded = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    name = "LizardGPU_decompressSeekableStream_device" if seek else "LizardGPU_decompressStream_device"
    r = getattr(L, name)(dst.data_ptr(), int(dst.numel()), src.data_ptr(), int(src.numel()), ctypes.byref(used), ctypes.byref(frames),
                         ctypes.byref(decoded), 0 if verify_checksum else FRAME_SKIP_CHECKSUM, stream)
    if L.LizardGPU_frameIsError(r):
        raise _lib.LizardAmdError(f"{name}: frame {frames.value} at offset {used.value}: "
                                  f"{L.LizardF_getErrorName(r).decode()} ({L.LizardGPU_lastError().decode()})")
    return dst[:r], frames.value


def _decompress_stream_items_device(src, items, size, verify_checksum=True):
    """LizardGPU_decompressStreamItems_device: the items `items` (strictly ascending indices into the seek table) of the seekable stream
    in `src` decoded back to back into one new uint8 CUDA tensor of `size` bytes, on torch's current stream."""
    import torch
    L = _lib.lib()
    n = len(items)
    dst = torch.empty(max(int(size), 1), dtype=torch.uint8, device=src.device)[:int(size)]
    L.LizardGPU_setDevice(src.device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    failed = ctypes.c_size_t(0)
    r = L.LizardGPU_decompressStreamItems_device(dst.data_ptr(), int(dst.numel()), src.data_ptr(), int(src.numel()), (ctypes.c_size_t * max(n, 1))(*items), n,
                                                 None, ctypes.byref(failed), 0 if verify_checksum else FRAME_SKIP_CHECKSUM, stream)
    if L.LizardGPU_frameIsError(r):
        raise _lib.LizardAmdError(f"LizardGPU_decompressStreamItems_device: {L.LizardF_getErrorName(r).decode()} ({L.LizardGPU_lastError().decode()})")
    return dst[:r]


def decompress_stream_items_device(src, items, verify_checksum=True):
    """Only the listed items of the seekable stream in `src` (a contiguous uint8 CUDA tensor): `items` are strictly ascending indices
    into its seek table.  A list of uint8 CUDA views into one allocation, one per listed item.  Raises LizardAmdError for a stream
    without a usable seek table, an index out of range or not ascending, and for an item whose frame does not answer its entry."""
    import torch
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    items = [int(k) for k in items]
    if not items:
        return []
    table = stream_seek_table_device(src)
    sizes = [table[k]["decoded_bytes"] if table is not None and 0 <= k < len(table) else 0 for k in items]
    out = _decompress_stream_items_device(src, items, sum(sizes), verify_checksum)
    views, at = [], 0
    for n in sizes:
        views.append(out[at:at + n])
        at += n
    return views


# ---- tensor streams: element bytes split into planes before compressing (include/lizard_amd.h Part 3c) ----

TENSOR_HEADER_MAX = 8 + 40 + 8 * 8          # bytes of the longest "LZT1" / "LZT2" tensor header (ndim = 8)
TENSOR_HEADER3_MAX = 8 + 48 + 8 * 8         # ... and of the longest "LZT3" header, the longest a reader meets
TENSOR_XOR_BASE = 1                         # LIZARDGPU_TENSOR_XOR_BASE: the flag of an "LZT3" header


FILTER_BYTE_PLANES, FILTER_BIT_PLANES = 0, 1   # LIZARDGPU_FILTER_*: what a tensor header says its data frame's bytes were split with
_PLANES_NAMES = {FILTER_BYTE_PLANES: "bytes", FILTER_BIT_PLANES: "bits"}


class _TensorDesc(ctypes.Structure):
    """LizardGPU_tensorDesc2_t: the v1 fields, then the filter."""
    _fields_ = [("elemSize", ctypes.c_uint32), ("ndim", ctypes.c_uint32), ("nbytes", ctypes.c_uint64), ("shape", ctypes.c_uint64 * 8),
                ("dtype", ctypes.c_char * 24), ("filter", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class _TensorDesc3(ctypes.Structure):
    """LizardGPU_tensorDesc3_t: the v2 fields with `reserved` named `flags`, then the base's tag."""
    _fields_ = [("elemSize", ctypes.c_uint32), ("ndim", ctypes.c_uint32), ("nbytes", ctypes.c_uint64), ("shape", ctypes.c_uint64 * 8),
                ("dtype", ctypes.c_char * 24), ("filter", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("baseTag", ctypes.c_uint64)]


def _as_bytes(t):
    """The bytes of a contiguous tensor of any dtype and rank as a flat uint8 view."""
    import torch
    return t.reshape(-1).view(torch.uint8)


def _plane_elem_size(t):
    """The element size a tensor's bytes are split with: element_size(), the size of one PART for a complex dtype (4 for complex64,
    8 for complex128), never more than 8."""
    e = t.element_size()
    if t.is_complex():
        e //= 2
    return min(e, 8)


def _planes_device(tensors, elem_sizes, join, filters=FILTER_BYTE_PLANES, bases=None, xor_entry=None):
    """`filters`: one LIZARDGPU_FILTER_* for all tensors or one per tensor; ONE launch per filter that occurs, all into one output
    tensor.  `xor_entry` (one bool per tensor; None: none): the tensors that go through LizardGPU_splitPlanesXor_device /
    LizardGPU_joinPlanesXor_device with bases[i] (None: no base) — one more launch per filter that occurs among THEM, into the same
    output tensor; the others take the plain entries as before."""
    import torch
    L = _lib.lib()
    tensors = list(tensors)
    if not tensors:
        return []
    device = tensors[0].device
    for t in tensors:
        assert t.is_cuda and t.is_contiguous() and t.device == device
    n = len(tensors)
    if elem_sizes is None:
        elem_sizes = [_plane_elem_size(t) for t in tensors]
    elem_sizes = [int(e) for e in elem_sizes]
    assert len(elem_sizes) == n
    filters = [filters] * n if isinstance(filters, int) else [int(f) for f in filters]
    assert len(filters) == n and all(f in _PLANES_NAMES for f in filters)
    xor_entry = [False] * n if xor_entry is None else [bool(x) for x in xor_entry]
    bases = [None] * n if bases is None else list(bases)
    assert len(xor_entry) == n and len(bases) == n
    sizes = [int(t.numel()) * t.element_size() for t in tensors]
    for i, b in enumerate(bases):
        if b is not None:
            assert xor_entry[i] and b.is_cuda and b.is_contiguous() and b.device == device and int(b.numel()) * b.element_size() == sizes[i]
    offsets, total = [], 0
    for s in sizes:
        offsets.append(total)
        total += (s + 255) & ~255
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    L.LizardGPU_setDevice(device.index or 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    for f in sorted(set(filters)):
        name = "LizardGPU_%s%sPlanes_device" % ("join" if join else "split", "Bit" if f == FILTER_BIT_PLANES else "")
        pick = [i for i in range(n) if filters[i] == f and not xor_entry[i]]
        k = len(pick)
        if k:
            srcs = (ctypes.c_void_p * k)(*[tensors[i].data_ptr() for i in pick])
            dsts = (ctypes.c_void_p * k)(*[out.data_ptr() + offsets[i] for i in pick])
            _lib.check(getattr(L, name)(k, dsts, srcs, (ctypes.c_size_t * k)(*[sizes[i] for i in pick]),
                                        (ctypes.c_uint32 * k)(*[elem_sizes[i] for i in pick]), stream), name)
        pick = [i for i in range(n) if filters[i] == f and xor_entry[i]]
        k = len(pick)
        if k:
            name = "LizardGPU_%sPlanesXor_device" % ("join" if join else "split")
            srcs = (ctypes.c_void_p * k)(*[tensors[i].data_ptr() for i in pick])
            dsts = (ctypes.c_void_p * k)(*[out.data_ptr() + offsets[i] for i in pick])
            xors = (ctypes.c_void_p * k)(*[None if bases[i] is None else bases[i].data_ptr() for i in pick])
            _lib.check(getattr(L, name)(k, dsts, srcs, xors, (ctypes.c_size_t * k)(*[sizes[i] for i in pick]),
                                        (ctypes.c_uint32 * k)(*[elem_sizes[i] for i in pick]), f, stream), name)
    return [out[o:o + s] for o, s in zip(offsets, sizes)]


def split_planes_device(tensors, elem_sizes=None):
    """The bytes of `tensors` — contiguous CUDA tensors of any dtype on one device, taken as bytes — regrouped by significance in ONE
    launch of LizardGPU_splitPlanes_device on torch's current stream: for a tensor of n elements of E bytes, all byte 0 of every
    element, then all byte 1, ... (dst[p * n + i] = src[i * E + p]; bytes behind the last whole element are copied).  `elem_sizes`
    (1, 2, 4 or 8 each) defaults to every tensor's element_size(), the size of one part for a complex dtype (4 for complex64, 8 for
    complex128).  Returns uint8 views into ONE output tensor, at 256-byte-aligned offsets."""
    return _planes_device(tensors, elem_sizes, False)


def join_planes_device(tensors, elem_sizes):
    """The inverse of split_planes_device for the same `elem_sizes`, in ONE launch of LizardGPU_joinPlanes_device: uint8 views into one
    output tensor, at 256-byte-aligned offsets."""
    return _planes_device(tensors, elem_sizes, True)


def split_bit_planes_device(tensors, elem_sizes=None):
    """The BITS of `tensors` regrouped by weight in ONE launch of LizardGPU_splitBitPlanes_device on torch's current stream — the twin
    of split_planes_device, same arguments and result: for a tensor of n elements of E bytes, all bit 0 of every element, then all
    bit 1, ... (include/lizard_amd.h Part 3c: dst[k * P + j] holds bit k of elements 8 j .. 8 j + 7, P = (n - n % 8) / 8; the last
    n % 8 elements and the bytes behind the last whole element are copied).  An element size of 1 is NOT a copy: eight planes.
    Returns uint8 views into ONE output tensor, at 256-byte-aligned offsets."""
    return _planes_device(tensors, elem_sizes, False, FILTER_BIT_PLANES)


def join_bit_planes_device(tensors, elem_sizes):
    """The inverse of split_bit_planes_device for the same `elem_sizes`, in ONE launch of LizardGPU_joinBitPlanes_device: uint8 views
    into one output tensor, at 256-byte-aligned offsets."""
    return _planes_device(tensors, elem_sizes, True, FILTER_BIT_PLANES)


def _planes_filter(planes, what):
    if planes not in ("bytes", "bits"):
        raise ValueError(f"{what}: planes={planes!r} is neither 'bytes' nor 'bits'")
    return FILTER_BIT_PLANES if planes == "bits" else FILTER_BYTE_PLANES


def split_planes_xor_device(tensors, bases, elem_sizes=None, planes="bytes"):
    """split_planes_device (planes="bytes") or split_bit_planes_device (planes="bits") of `tensors` XOR `bases`, in ONE launch of
    LizardGPU_splitPlanesXor_device on torch's current stream: every tensor's bytes are XORed with the bytes of its base in registers
    on their way into the planes — no third buffer, 3 bytes of memory traffic per payload byte.  `bases`: a list as long as `tensors`
    of contiguous CUDA tensors on the same device with the tensor's byte size, an earlier version of each tensor; bases[i] may be
    None: tensor i is split as it is, in the same launch.  XOR against an earlier version turns every unchanged bit into a zero and
    the planes put those zeros into runs: use it only against a base the data derives from (include/lizard_amd.h Part 3c has the
    table).  Returns uint8 views into ONE output tensor, at 256-byte-aligned offsets."""
    tensors, bases = list(tensors), list(bases)
    if len(bases) != len(tensors):
        raise ValueError(f"split_planes_xor_device: {len(bases)} bases for {len(tensors)} tensors")
    return _planes_device(tensors, elem_sizes, False, _planes_filter(planes, "split_planes_xor_device"), bases, [True] * len(tensors))


def join_planes_xor_device(tensors, bases, elem_sizes, planes="bytes"):
    """The inverse of split_planes_xor_device for the same `bases`, `elem_sizes` and `planes`, in ONE launch of
    LizardGPU_joinPlanesXor_device: join(tensor) XOR base; uint8 views into one output tensor, at 256-byte-aligned offsets."""
    tensors, bases = list(tensors), list(bases)
    if len(bases) != len(tensors):
        raise ValueError(f"join_planes_xor_device: {len(bases)} bases for {len(tensors)} tensors")
    return _planes_device(tensors, elem_sizes, True, _planes_filter(planes, "join_planes_xor_device"), bases, [True] * len(tensors))


def compress_tensors_device(tensors, level=LIZARD_MIN_CLEVEL, block_size_id=0, checksum=False, split=True, planes="bytes", base=None,
                            base_tag=0, seekable=False):
    """A .liz STREAM for `tensors`, contiguous CUDA tensors of any dtype and shape on one device (zero-element ones and scalars
    allowed), as ONE uint8 CUDA tensor: per tensor a tensor header — a skippable frame with the dtype's name, the shape and the
    element size of the split (LizardGPU_tensorHeaderWrite) — and one frame with content size over the tensor's bytes SPLIT INTO
    PLANES.  Every decoder of the format reads the stream (the headers are skipped, the frames decode to the split bytes);
    decompress_tensors_device gives the tensors back.
    What the split is for: interleaved, the exponent byte of a float is hidden from a byte-oriented parser and from huff0 — bf16 or
    fp32 weights come out of compress_stream_device at their own size — and in a plane of its own it has under 3 bits.  With byte
    planes fp16 gains nothing at these levels (its top byte holds 5.5 bits and the Huffman stage stores it raw).
    planes="bits" (opt-in; the default and every call without it produce the same stream bytes as before): EVERY tensor, element
    size 1 included (a bool mask holds one used bit of eight), goes through one split_bit_planes_device launch with
    _plane_elem_size(t) and gets an "LZT2" header (LizardGPU_tensorHeaderWrite2, filter LIZARDGPU_FILTER_BIT_PLANES), which readers
    of "LZT1" refuse.  A nearly constant bit plane is a long run that the LZ parser alone removes: fp16 weights shrink at all
    (0.94 of raw), and bf16 / fp32 weights reach level 30's ratio at level 10 (0.76 against 0.84 for bf16).  Bit planes lose
    against byte planes for activation-like bf16 (randn * 1.0) and for bf16 / fp32 weights at levels 30 and above: include/lizard_amd.h
    has the table.  planes="bits" with split=False, or another value of `planes`, raises ValueError.
    In this order: one split launch (split_planes_device) for the tensors whose element size is above 1 — none with split=False,
    which compresses every tensor's own bytes and records element size 1 —, all headers written into one host buffer, ONE call of
    LizardGPU_compressStream_device over all tensors with the headers as its prefixes (compress_stream_device_into), which writes
    every header and every frame once, to its place.  No payload byte crosses PCIe.
    Memory: the split bytes are a temporary of the size of the batch, beside the one allocation of LizardGPU_compressStreamBound bytes
    of which the result is a view.
    base (opt-in, per tensor; without it the call is what it was, byte for byte): a list as long as `tensors` whose entries are None
    or a contiguous CUDA tensor on the same device with the tensor's dtype and shape (else ValueError naming the index) — an EARLIER
    VERSION of the tensor that the reader will hold too: the previous checkpoint, the base model of a fine-tune.  The tensors with
    a base, element size 1 included, go through ONE split_planes_xor_device launch (`planes` chooses the layout), which XORs each
    with its base on the way into the planes — no temporary beyond the split buffer — and get an "LZT3" header
    (LizardGPU_tensorHeaderWrite3) that holds `base_tag`, an opaque number of the caller's (a step number, a hash of their own)
    by which a reader learns that it was handed the wrong base; the library does not hash bases.  The tensors without a base take
    the path and the headers above.  Unchanged bits become zeros and the planes put them into runs: bf16 weights one Adam step of
    lr 1e-5 behind their base are 0.31 of raw at level 10 and 0.15 at level 30 (0.84 / 0.75 without).  Use it only against a base
    the data derives from: with an unrelated base it LOSES at level 10 with byte planes (0.91 against 0.84).  Readers of "LZT1" /
    "LZT2" refuse "LZT3".  base with split=False raises ValueError.
    seekable=True (opt-in; without it the bytes are what they were): the same stream with a seek table behind the last tensor
    (compress_stream_device_into), one entry per tensor with the tensor header as its prefix.  decompress_tensors_device(seek=True)
    then finds headers and frames without a walk, and select=[...] decodes some tensors only; readers that do not know the table
    step over it."""
    L = _lib.lib()
    if planes not in ("bytes", "bits"):
        raise ValueError(f"compress_tensors_device: planes={planes!r} is neither 'bytes' nor 'bits'")
    if planes == "bits" and not split:
        raise ValueError("compress_tensors_device: planes='bits' with split=False (bit planes are a split)")
    if base is not None and not split:
        raise ValueError("compress_tensors_device: base with split=False (the XOR with a base is a filter of the split)")
    bits = planes == "bits"
    tensors = list(tensors)
    if not tensors:
        raise ValueError("compress_tensors_device: no tensors")
    device = tensors[0].device
    base = [None] * len(tensors) if base is None else list(base)
    if len(base) != len(tensors):
        raise ValueError(f"compress_tensors_device: {len(base)} bases for {len(tensors)} tensors")
    for i, (t, b) in enumerate(zip(tensors, base)):
        if b is not None and (b.dtype != t.dtype or tuple(b.shape) != tuple(t.shape)):
            raise ValueError(f"compress_tensors_device: tensor {i}: its base is {b.dtype} {tuple(b.shape)}, the tensor {t.dtype} {tuple(t.shape)}")
        if b is not None and not (b.is_cuda and b.is_contiguous() and b.device == device):
            raise ValueError(f"compress_tensors_device: tensor {i}: its base is not a contiguous CUDA tensor on {device}")
    descs = []
    for i, t in enumerate(tensors):
        assert t.is_cuda and t.is_contiguous() and t.device == device
        name = str(t.dtype).split(".")[-1].encode()
        if t.dim() > 8 or len(name) > 23:
            raise _lib.LizardAmdError(f"compress_tensors_device: tensor {i}: {t.dim()} dimensions / dtype {name.decode()} do not fit a tensor header")
        d = _TensorDesc3()
        d.elemSize, d.ndim, d.nbytes, d.dtype = (_plane_elem_size(t) if split else 1), t.dim(), int(t.numel()) * t.element_size(), name
        d.filter = FILTER_BIT_PLANES if bits else FILTER_BYTE_PLANES
        if base[i] is not None:
            d.flags, d.baseTag = TENSOR_XOR_BASE, int(base_tag)
        for k, s in enumerate(t.shape):
            d.shape[k] = int(s)
        descs.append(d)
    raw = [_as_bytes(t) for t in tensors]
    # what is split: with bit planes every tensor, with byte planes those wider than a byte — and every tensor that has a base
    wide = [i for i, d in enumerate(descs) if bits or d.elemSize > 1 or base[i] is not None]
    if wide:
        for i, p in zip(wide, _planes_device([raw[i] for i in wide], [descs[i].elemSize for i in wide], False, descs[0].filter,
                                             [None if base[i] is None else _as_bytes(base[i]) for i in wide],
                                             [base[i] is not None for i in wide])):
            raw[i] = p
    host = np.zeros(len(descs) * TENSOR_HEADER3_MAX, dtype=np.uint8)
    at, headers = 0, []
    for i, d in enumerate(descs):
        n = L.LizardGPU_tensorHeaderWrite3(host.ctypes.data + at, host.size - at, ctypes.byref(d))
        if not n:
            raise _lib.LizardAmdError(f"compress_tensors_device: tensor {i}: LizardGPU_tensorHeaderWrite3 refused the descriptor")
        headers.append(host[at:at + n].tobytes())
        at += n
    return compress_stream_device_into(raw, None, headers, level, block_size_id, checksum, True, seekable)[0]


SEEK_MAGIC = 0x184D2A5E                     # LIZARDGPU_SEEK_MAGIC: the skippable frame that holds a seek table


def _tensor_stream_pairs_seek(src, what, select):
    """The (tensor header, data frame) pairs from the stream's seek table, in the keys of stream_info_device that the tensor entries use;
    with `select` those tensors only.  (pairs, tensors in the stream)"""
    table = stream_seek_table_device(src)
    if table is None:
        raise _lib.LizardAmdError(f"{what}: the stream has no usable seek table (write it with seekable=True, or read it without seek / select)")
    picked = range(len(table)) if select is None else select
    pairs = []
    for j, k in enumerate(picked):
        if not 0 <= k < len(table):
            raise _lib.LizardAmdError(f"{what}: select[{j}] = {k}, the stream has {len(table)} tensors")
        if j and k <= picked[j - 1]:
            raise _lib.LizardAmdError(f"{what}: select[{j}] = {k} does not ascend from select[{j - 1}] = {picked[j - 1]}")
        e = table[k]
        if not e["prefix_bytes"]:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: the data frame at offset {e['offset']} has no tensor header in front of it")
        pairs.append(({"offset": e["offset"], "frame_bytes": e["prefix_bytes"]},
                      {"offset": e["offset"] + e["prefix_bytes"], "frame_bytes": e["frame_bytes"], "content_size": e["decoded_bytes"],
                       "n_records": 1 if e["decoded_bytes"] else 0}))
    return pairs, len(table)


def _tensor_stream_index(src, what, seek=False, select=None):
    """The (tensor header, data frame) pairs of the tensor stream in `src`: one stream_info_device — with `seek` the stream's seek
    table instead, and no walk —, one indexed read of all header bytes.  ([(header frame, data frame, descriptor)], tensors in the
    stream): with `select` (ascending indices; implies seek) the list holds those tensors only."""
    if seek or select is not None:
        pairs, count = _tensor_stream_pairs_seek(src, what, select)
        return _tensor_stream_headers(src, what, pairs, range(count) if select is None else select), count
    frames = stream_info_device(src)
    if len(frames) % 2 and frames[-1]["skippable"] and frames[-1]["frame_bytes"] >= 48 \
            and int.from_bytes(bytes(src[frames[-1]["offset"]:frames[-1]["offset"] + 4].cpu().numpy()), "little") == SEEK_MAGIC:
        frames.pop()                                           # a seekable stream read by the walk: its table is not a tensor
    pairs, i = [], 0
    while i < len(frames):
        k, f = len(pairs), frames[i]
        if not f["skippable"]:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: the data frame at offset {f['offset']} has no tensor header in front of it")
        if i + 1 == len(frames) or frames[i + 1]["skippable"]:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: the skippable frame at offset {f['offset']} is not followed by a data frame")
        pairs.append((f, frames[i + 1]))
        i += 2
    return _tensor_stream_headers(src, what, pairs, range(len(pairs))), len(pairs)


def _tensor_stream_headers(src, what, pairs, numbers):
    """The descriptors of the tensor headers in front of `pairs`, tensors `numbers` of the stream: one indexed read of all header bytes."""
    import torch
    L = _lib.lib()
    if not pairs:
        return []
    takes = [min(h["frame_bytes"], TENSOR_HEADER3_MAX) for h, _ in pairs]
    index = np.concatenate([np.arange(h["offset"], h["offset"] + n, dtype=np.int64) for (h, _), n in zip(pairs, takes)])
    host = np.ascontiguousarray(src[torch.from_numpy(index).to(src.device)].cpu().numpy())
    out, at = [], 0
    for k, (h, f), n in zip(numbers, pairs, takes):
        d, used = _TensorDesc3(), ctypes.c_size_t(0)
        rc = L.LizardGPU_tensorHeaderRead3(host.ctypes.data + at, n, ctypes.byref(d), ctypes.byref(used))
        if rc or used.value != h["frame_bytes"]:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: the skippable frame at offset {h['offset']} in front of the data frame is not a "
                                      f"tensor header, so the data frame at offset {f['offset']} has no tensor header in front of it")
        at += n
        out.append((h, f, d))
    return out


def tensors_info_device(stream, seek=False):
    """What the tensor stream in `stream` (a contiguous uint8 CUDA tensor, what compress_tensors_device returns) holds, without
    decoding anything: one dict per tensor with dtype (its name), shape, planes ("bytes" or "bits": the filter), elem_size (of the
    split; with "bytes", 1 = stored unsplit), nbytes, offset (of the tensor's header in the stream), header_bytes and frame_bytes (of the data frame behind the header),
    xor_base (bool: an "LZT3" header — the tensor was XORed with a base, which decompress_tensors_device needs) and base_tag (the
    number the writer stored for that base; 0 without one).  Raises
    LizardAmdError naming the tensor's index for a data frame without a tensor header in front of it.  A seek table behind the last
    tensor is not a tensor.  seek=True takes the places from the stream's seek table instead of a walk, and raises LizardAmdError
    when the stream has no usable one."""
    return [{"dtype": d.dtype.decode(), "shape": tuple(int(s) for s in d.shape[:d.ndim]), "planes": _PLANES_NAMES[int(d.filter)],
             "elem_size": int(d.elemSize), "nbytes": int(d.nbytes), "xor_base": bool(d.flags & TENSOR_XOR_BASE), "base_tag": int(d.baseTag),
             "offset": h["offset"], "header_bytes": h["frame_bytes"], "frame_bytes": f["frame_bytes"]}
            for h, f, d in _tensor_stream_index(stream, "tensors_info_device", seek)[0]]


def decompress_tensors_device(stream, verify_checksum=True, base=None, base_tag=None, seek=False, select=None):
    """The tensors of the tensor stream in `stream`, a contiguous uint8 CUDA tensor (what compress_tensors_device returns), with dtype
    and shape restored: a list of views into ONE allocation, each 256-byte aligned.  In this order: one stream_info_device, one
    indexed read of all header bytes, one decompress_stream_device — ONE decode batch for a stream of this library, because the headers
    are skippable frames and every data frame carries its content size — and one join launch per filter that occurs in the stream
    (byte planes, bit planes: a stream may mix both kinds of tensor), at most two, into the one result.  No payload byte crosses
    PCIe.
    Raises LizardAmdError naming the index of the offending tensor when a data frame has no tensor header in front of it (or a
    skippable frame that is none), when a header's nbytes differs from its frame's decoded size (a data frame with records must
    carry its content size), when the shape does not make nbytes, or when torch does not know the dtype's name; a frame the decoder
    refuses raises as in decompress_stream_device.
    Memory: the decoded, still split bytes are a temporary of the size of the batch beside the result.
    base: what compress_tensors_device was given — a list indexed by the tensor's position in the stream, as long as the stream has
    tensors (else ValueError), of None or a contiguous CUDA tensor on the stream's device.  A tensor with an "LZT3" header is joined
    and XORed with its base (join_planes_xor_device's kernel: one more launch per filter that occurs among such tensors, into the
    same result); a stream without one takes exactly the path above.  Raises LizardAmdError naming the tensor's index when an
    "LZT3" tensor has no base, when its base's byte size or dtype is not the header's, or when `base_tag` is given and differs
    from the header's.  A base handed for a tensor whose header is not "LZT3" is IGNORED.  The library cannot tell a wrong base
    of the right size and tag: the tensor then comes back wrong, silently — the tag is the caller's guard.
    A seekable stream (compress_tensors_device(..., seekable=True)) reads like any other here: the table behind the last tensor is
    stepped over.  seek=True takes the places of headers and frames from that table — no stream_info_device, no walk in the decode
    (decompress_stream_device(seek=True)) — and raises LizardAmdError when the stream has no usable one.  select=[indices] (strictly
    ascending positions in the stream; implies seek) decodes ONLY those tensors, through LizardGPU_decompressStreamItems_device, and
    returns them in that order; `base` stays indexed by position in the stream and as long as the stream has tensors."""
    import torch
    what = "decompress_tensors_device"
    select = None if select is None else [int(k) for k in select]
    entries, count = _tensor_stream_index(stream, what, seek, select)
    numbers = list(range(count)) if select is None else select
    if base is not None:
        base = list(base)
        if len(base) != count:
            raise ValueError(f"{what}: {len(base)} bases for a stream of {count} tensors")
    if not entries:
        return []
    dtypes = []
    for k, (h, f, d) in zip(numbers, entries):
        known = f["content_size"] if f["n_records"] else 0
        if f["n_records"] and not f["content_size"]:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: the data frame at offset {f['offset']} carries no content size")
        if known != d.nbytes:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: the header says {d.nbytes} bytes, the frame at offset {f['offset']} decodes to {known}")
        dt = getattr(torch, d.dtype.decode(errors="replace"), None)
        if not isinstance(dt, torch.dtype):
            raise _lib.LizardAmdError(f"{what}: tensor {k}: torch knows no dtype {d.dtype.decode(errors='replace')!r}")
        count = int(np.prod([int(s) for s in d.shape[:d.ndim]], dtype=object)) if d.ndim else 1
        if count * torch.empty(0, dtype=dt).element_size() != d.nbytes:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: shape {tuple(d.shape[:d.ndim])} of {d.dtype.decode()} is not {d.nbytes} bytes")
        dtypes.append(dt)
        if d.flags & TENSOR_XOR_BASE:
            b = None if base is None else base[k]
            if b is None:
                raise _lib.LizardAmdError(f"{what}: tensor {k}: its header says it was XORed with a base (tag {d.baseTag}), and none was given")
            if int(b.numel()) * b.element_size() != d.nbytes or b.dtype != dt:
                raise _lib.LizardAmdError(f"{what}: tensor {k}: its base is {int(b.numel()) * b.element_size()} bytes of {b.dtype}, "
                                          f"the header says {d.nbytes} bytes of {dt}")
            if base_tag is not None and int(base_tag) != d.baseTag:
                raise _lib.LizardAmdError(f"{what}: tensor {k}: the header holds base tag {d.baseTag}, the caller gave {int(base_tag)}")
            if not (b.is_cuda and b.is_contiguous() and b.device == stream.device):
                raise _lib.LizardAmdError(f"{what}: tensor {k}: its base is not a contiguous CUDA tensor on {stream.device}")
    total = sum(int(d.nbytes) for _, _, d in entries)
    if select is None:
        decoded, _ = decompress_stream_device(stream, size=total, verify_checksum=verify_checksum, seek=seek)
    else:
        decoded = _decompress_stream_items_device(stream, select, total, verify_checksum)
    if int(decoded.numel()) != total:
        raise _lib.LizardAmdError(f"{what}: the stream decoded to {int(decoded.numel())} bytes, its headers say {total}")
    pieces, pos = [], 0
    for _, _, d in entries:
        pieces.append(decoded[pos:pos + int(d.nbytes)])
        pos += int(d.nbytes)
    xored = [bool(d.flags & TENSOR_XOR_BASE) for _, _, d in entries]
    joined = _planes_device(pieces, [int(d.elemSize) for _, _, d in entries], True, [int(d.filter) for _, _, d in entries],
                            [_as_bytes(base[k]) if x else None for k, x in zip(numbers, xored)] if any(xored) else None, xored)
    return [b.view(dt).reshape(tuple(int(s) for s in d.shape[:d.ndim])) for b, dt, (_, _, d) in zip(joined, dtypes, entries)]


class _ByteRange(ctypes.Structure):
    """LizardGPU_byteRange_t."""
    _fields_ = [("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64)]


class _SliceFrame(ctypes.Structure):
    """LizardGPU_sliceFrame_t."""
    _fields_ = [("d_src", ctypes.c_void_p), ("srcSize", ctypes.c_size_t), ("firstRange", ctypes.c_uint32), ("nRanges", ctypes.c_uint32)]


class _PlanesRange(ctypes.Structure):
    """LizardGPU_planesRange_t."""
    _fields_ = [("d_dst", ctypes.c_void_p), ("d_base", ctypes.c_void_p), ("nElems", ctypes.c_uint64), ("first", ctypes.c_uint64),
                ("last", ctypes.c_uint64), ("elemSize", ctypes.c_uint32), ("filter", ctypes.c_uint32), ("firstPiece", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def planes_range_bytes(n_elems, elem_size, planes, first, last):
    """LizardGPU_planesRangeBytes: the byte ranges [(lo, hi)] of the SPLIT content that elements [first, last) of a buffer of n_elems
    elements of elem_size bytes need, in piece order; planes is "bytes" or "bits".  ValueError for arguments the entry refuses."""
    L = _lib.lib()
    out = (_ByteRange * 65)()
    n = L.LizardGPU_planesRangeBytes(int(n_elems), int(elem_size), _planes_filter(planes, "planes_range_bytes"), int(first), int(last), out, 65)
    if not n:
        raise ValueError(f"planes_range_bytes: elements [{first}, {last}) of {n_elems} elements of {elem_size} bytes")
    return [(int(r.lo), int(r.hi)) for r in out[:n]]


def decompress_tensor_slices_device(stream, slices, base=None, base_tag=None):
    """Rows [start, stop) of some tensors of the SEEKABLE tensor stream in `stream` (a contiguous uint8 CUDA tensor, what
    compress_tensors_device(..., seekable=True) returns), decoding only the blocks that cover them.  `slices`: a list of
    (k, start, stop) with k a position in the stream, strictly ascending, and 0 <= start <= stop <= shape[0].  Tensor j of the result
    equals decompress_tensors_device(stream, select=[k], base=base, base_tag=base_tag)[0][start:stop] — dtype, shape
    (stop - start, *shape[1:]) and every bit — and the result is a list of views into ONE allocation, each 256-byte aligned.
    What a tensor-parallel loader does with the whole-tensor entry is decode all of every tensor — the split bytes as a temporary, then
    the joined tensor — and throw most of it away; here the temporary holds the covering blocks of the range's byte ranges alone (per
    plane at most two blocks more than the range's share) and the result the range alone.
    In this order: the seek table; one indexed read of the picked tensor headers; one LizardGPU_framesInfo_device over the picked data
    frames, for their block sizes; the byte ranges and their bound on the host (LizardGPU_planesRangeBytes, LizardGPU_frameRangesBound);
    ONE LizardGPU_decompressFrameRanges_device; ONE LizardGPU_joinPlanesRange_device.  No payload byte crosses PCIe.  A stream may mix
    "LZT1", "LZT2" and "LZT3" tensors, split or not.
    base: as in decompress_tensors_device — a list indexed by position in the stream, as long as the stream has tensors, of None or the
    WHOLE base tensor; the slice of the base is taken inside the call.  base_tag as there.
    ValueError: a 0-dim tensor, start / stop out of order or out of range, positions that do not ascend, a base list of another length.
    LizardAmdError naming the tensor: a stream without a usable seek table, a frame the slice decoder refuses, a missing or mismatched
    base, a wrong tag, a header that does not fit its frame — the messages of decompress_tensors_device where the case is the same.
    LIMITS (include/lizard_amd.h Part 3d): a frame's content checksum is never verified here, because a slice cannot verify it; damage
    in a block that is not picked is not seen; the frames must have independent blocks that all but the last fill the block size,
    which is every frame this library writes.  Column ranges and other strided slices are out of scope."""
    import torch
    what = "decompress_tensor_slices_device"
    L = _lib.lib()
    slices = [(int(k), int(a), int(b)) for k, a, b in slices]
    for j in range(1, len(slices)):
        if slices[j][0] <= slices[j - 1][0]:
            raise ValueError(f"{what}: slices[{j}] names tensor {slices[j][0]}, which does not ascend from slices[{j - 1}]'s {slices[j - 1][0]}")
    numbers = [k for k, _, _ in slices]
    entries, count = _tensor_stream_index(stream, what, True, numbers)
    if base is not None:
        base = list(base)
        if len(base) != count:
            raise ValueError(f"{what}: {len(base)} bases for a stream of {count} tensors")
    if not entries:
        return []
    device = stream.device
    plans = []                                                  # (dtype, shape, E, filter, n elements, first, last, row bytes, base or None)
    for (k, start, stop), (h, f, d) in zip(slices, entries):
        if f["content_size"] != d.nbytes:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: the header says {d.nbytes} bytes, the frame at offset {f['offset']} decodes to {f['content_size']}")
        dt = getattr(torch, d.dtype.decode(errors="replace"), None)
        if not isinstance(dt, torch.dtype):
            raise _lib.LizardAmdError(f"{what}: tensor {k}: torch knows no dtype {d.dtype.decode(errors='replace')!r}")
        shape = tuple(int(s) for s in d.shape[:d.ndim])
        n_items = int(np.prod(shape, dtype=object)) if d.ndim else 1
        if n_items * torch.empty(0, dtype=dt).element_size() != d.nbytes:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: shape {shape} of {d.dtype.decode()} is not {d.nbytes} bytes")
        if not d.ndim:
            raise ValueError(f"{what}: tensor {k} has no dimension to slice")
        if not 0 <= start <= stop <= shape[0]:
            raise ValueError(f"{what}: tensor {k}: rows [{start}, {stop}) of {shape[0]}")
        E = int(d.elemSize)
        row = int(d.nbytes) // shape[0] if shape[0] else 0     # (a multiple of E: E divides the dtype's element size)
        b = None
        if d.flags & TENSOR_XOR_BASE:
            b = None if base is None else base[k]
            if b is None:
                raise _lib.LizardAmdError(f"{what}: tensor {k}: its header says it was XORed with a base (tag {d.baseTag}), and none was given")
            if int(b.numel()) * b.element_size() != d.nbytes or b.dtype != dt:
                raise _lib.LizardAmdError(f"{what}: tensor {k}: its base is {int(b.numel()) * b.element_size()} bytes of {b.dtype}, "
                                          f"the header says {d.nbytes} bytes of {dt}")
            if base_tag is not None and int(base_tag) != d.baseTag:
                raise _lib.LizardAmdError(f"{what}: tensor {k}: the header holds base tag {d.baseTag}, the caller gave {int(base_tag)}")
            if not (b.is_cuda and b.is_contiguous() and b.device == device):
                raise _lib.LizardAmdError(f"{what}: tensor {k}: its base is not a contiguous CUDA tensor on {device}")
        plans.append((dt, shape, E, int(d.filter), int(d.nbytes) // E, start * row // E, stop * row // E, row, b))
    n = len(plans)
    L.LizardGPU_setDevice(device.index or 0)
    hip_stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    # the block size of every picked data frame
    srcs = (ctypes.c_void_p * n)(*[stream.data_ptr() + f["offset"] for _, f, _ in entries])
    sizes = (ctypes.c_size_t * n)(*[f["frame_bytes"] for _, f, _ in entries])
    infos, codes = (_FrameInfo * n)(), (ctypes.c_int * n)()
    _lib.check(L.LizardGPU_framesInfo_device(n, srcs, sizes, infos, None, None, codes, hip_stream), "LizardGPU_framesInfo_device")
    for k, rc in zip(numbers, codes):
        if rc:
            raise _lib.LizardAmdError(f"{what}: tensor {k}: its data frame is refused: {L.LizardF_getErrorName((1 << 64) + rc).decode()}")
    # the byte ranges, their frames and the room their covering blocks take
    ranges, frames, bound = (_ByteRange * (65 * n))(), (_SliceFrame * n)(), 0
    at = 0
    for i, (_, _, E, filt, n_elems, first, last, _, _) in enumerate(plans):
        got = L.LizardGPU_planesRangeBytes(n_elems, E, filt, first, last, ctypes.byref(ranges, at * ctypes.sizeof(_ByteRange)), 65)
        if not got:
            raise _lib.LizardAmdError(f"{what}: tensor {numbers[i]}: LizardGPU_planesRangeBytes refused elements [{first}, {last}) of {n_elems}")
        frames[i].d_src, frames[i].srcSize, frames[i].firstRange, frames[i].nRanges = srcs[i], sizes[i], at, got
        bound += L.LizardGPU_frameRangesBound(ctypes.byref(ranges, at * ctypes.sizeof(_ByteRange)), got, L.LizardGPU_frameBlockSize(infos[i].blockSizeID))
        at += got
    scratch = torch.empty(max(bound, 1), dtype=torch.uint8, device=device)
    range_at, results = (ctypes.c_uint64 * (at + 1))(), (ctypes.c_size_t * n)()
    _lib.check(L.LizardGPU_decompressFrameRanges_device(scratch.data_ptr(), bound, n, frames, ranges, range_at, results, hip_stream),
               "LizardGPU_decompressFrameRanges_device")
    for k, r in zip(numbers, results):
        if L.LizardGPU_frameIsError(r):
            raise _lib.LizardAmdError(f"{what}: tensor {k}: its data frame is refused: {L.LizardF_getErrorName(r).decode()}")
    # the join of every range out of its pieces, into one result
    offsets, total = [], 0
    for _, _, E, _, _, first, last, _, _ in plans:
        offsets.append(total)
        total += ((last - first) * E + 255) & ~255
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    items, pieces = (_PlanesRange * n)(), (ctypes.c_void_p * at)()
    for i, ((k, start, _), (_, _, E, filt, n_elems, first, last, row, b)) in enumerate(zip(slices, plans)):
        B = L.LizardGPU_frameBlockSize(infos[i].blockSizeID)
        for q in range(frames[i].nRanges):
            r = frames[i].firstRange + q
            pieces[r] = scratch.data_ptr() + range_at[r] + ranges[r].lo % B
        it = items[i]
        it.d_dst, it.d_base = out.data_ptr() + offsets[i], None if b is None else _as_bytes(b).data_ptr() + start * row
        it.nElems, it.first, it.last, it.elemSize, it.filter, it.firstPiece = n_elems, first, last, E, filt, frames[i].firstRange
    _lib.check(L.LizardGPU_joinPlanesRange_device(n, items, pieces, hip_stream), "LizardGPU_joinPlanesRange_device")
    return [out[o:o + (last - first) * E].view(dt).reshape((stop - start,) + shape[1:])
            for o, (_, start, stop), (dt, shape, E, _, _, first, last, _, _) in zip(offsets, slices, plans)]
