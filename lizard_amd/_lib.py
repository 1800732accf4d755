"""ctypes binding of liblizard_amd.so (the C-ABI product library, include/lizard_amd.h).

There is no Python or CPU implementation behind this module: if the shared library has not been
built (`python -c "import __graft_entry__ as g; g.build()"` or `make -C lizard_amd/csrc`) importing
any compute entry point raises, loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblizard_amd.so")

_lib = None


class LizardAmdError(RuntimeError):
    pass


def build(force=False):
    """Compile liblizard_amd.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    args = ["make", "-C", os.path.join(_HERE, "csrc")]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LizardAmdError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. "
            "Run `make -C lizard_amd/csrc` (or __graft_entry__.build()). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    c = ctypes
    L.Lizard_versionNumber.restype = c.c_int
    L.Lizard_compressBound.argtypes = [c.c_int]; L.Lizard_compressBound.restype = c.c_int
    L.Lizard_sizeofState.argtypes = [c.c_int]; L.Lizard_sizeofState.restype = c.c_int
    L.Lizard_compress.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int]; L.Lizard_compress.restype = c.c_int
    L.Lizard_compress_extState.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int]
    L.Lizard_compress_extState.restype = c.c_int
    L.LizardGPU_levelSupported.argtypes = [c.c_int]; L.LizardGPU_levelSupported.restype = c.c_int
    L.LizardGPU_setDevice.argtypes = [c.c_int]; L.LizardGPU_setDevice.restype = c.c_int
    L.LizardGPU_lastError.restype = c.c_char_p
    L.LizardGPU_residentWaves.restype = c.c_int
    L.LizardGPU_lastKernelMs.restype = c.c_float
    L.LizardGPU_compressBlocks_device.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t, c.c_void_p,
                                                  c.c_size_t, c.c_void_p, c.c_int, c.c_void_p]
    L.LizardGPU_compressBlocks_device.restype = c.c_int
    L.LizardGPU_compressBlocks_host.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t, c.c_void_p,
                                                c.c_size_t, c.c_void_p, c.c_int]
    L.LizardGPU_compressBlocks_host.restype = c.c_int
    L.LizardGPU_compressBlocks_host_packed.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t, c.c_void_p,
                                                       c.c_size_t, c.c_void_p, c.c_void_p, c.c_int]
    L.LizardGPU_compressBlocks_host_packed.restype = c.c_int
    L.LizardGPU_maxBlockSize.argtypes = [c.c_int]; L.LizardGPU_maxBlockSize.restype = c.c_size_t
    L.LizardGPU_deviceCount.restype = c.c_int
    L.LizardGPU_shutdown.restype = None
    L.LizardGPU_shardRange.argtypes = [c.c_size_t, c.c_int, c.c_int, c.c_void_p, c.c_void_p]; L.LizardGPU_shardRange.restype = None
    L.LizardGPU_offsetsFromSizes.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p]; L.LizardGPU_offsetsFromSizes.restype = None
    L.LizardGPU_compressBlocks_sharded.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t,
                                                   c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_int]
    L.LizardGPU_compressBlocks_sharded.restype = c.c_int
    L.LizardGPU_commUniqueId.argtypes = [c.c_void_p]; L.LizardGPU_commUniqueId.restype = c.c_int
    L.LizardGPU_commInitRank.argtypes = [c.c_void_p, c.c_int, c.c_int]; L.LizardGPU_commInitRank.restype = c.c_int
    L.LizardGPU_gatherSizes_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_gatherSizes_device.restype = c.c_int
    L.LizardGPU_commDestroy.restype = c.c_int
    L.LizardGPU_decompressBlocks_host.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p]
    L.LizardGPU_decompressBlocks_host.restype = c.c_int
    L.LizardGPU_decompressBlocks_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t,
                                                    c.c_void_p, c.c_void_p]
    L.LizardGPU_decompressBlocks_device.restype = c.c_int
    L.LizardGPU_frameIsError.argtypes = [c.c_size_t]; L.LizardGPU_frameIsError.restype = c.c_uint
    L.LizardF_getErrorName.argtypes = [c.c_size_t]; L.LizardF_getErrorName.restype = c.c_char_p
    L.LizardGPU_compressFrameBound.argtypes = [c.c_size_t, c.c_void_p]; L.LizardGPU_compressFrameBound.restype = c.c_size_t
    L.LizardGPU_compressFrame.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p]
    L.LizardGPU_compressFrame.restype = c.c_size_t
    L.LizardGPU_decompressFrame.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p]
    L.LizardGPU_decompressFrame.restype = c.c_size_t
    L.LizardGPU_decompressFrameBound.argtypes = [c.c_void_p, c.c_size_t]; L.LizardGPU_decompressFrameBound.restype = c.c_size_t
    L.LizardGPU_frameIndex.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    L.LizardGPU_frameIndex.restype = c.c_int
    L.LizardGPU_frameDecodeStats.argtypes = [c.c_void_p]; L.LizardGPU_frameDecodeStats.restype = c.c_int
    L.LizardGPU_frameDecodePackedChunks.restype = c.c_ulonglong
    L.LizardGPU_decompressFrame_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_uint, c.c_void_p]
    L.LizardGPU_decompressFrame_device.restype = c.c_size_t
    L.LizardGPU_frameIndex_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p,
                                              c.c_void_p]
    L.LizardGPU_frameIndex_device.restype = c.c_int
    L.LizardGPU_frameWalkRecords.restype = c.c_size_t
    L.LizardGPU_frameBlockSize.argtypes = [c.c_uint]; L.LizardGPU_frameBlockSize.restype = c.c_size_t
    L.LizardGPU_frameDecodeDeviceStats.argtypes = [c.c_void_p]; L.LizardGPU_frameDecodeDeviceStats.restype = c.c_int
    L.LizardGPU_compressFrame_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    L.LizardGPU_compressFrame_device.restype = c.c_size_t
    L.LizardGPU_frameCompressDeviceStats.argtypes = [c.c_void_p]; L.LizardGPU_frameCompressDeviceStats.restype = c.c_int
    L.LizardGPU_compressFrames_device.argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_compressFrames_device.restype = c.c_int
    L.LizardGPU_compressStreamBound.argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_compressStreamBound.restype = c.c_size_t
    L.LizardGPU_compressStream_device.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                                  c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_compressStream_device.restype = c.c_size_t
    L.LizardGPU_streamCompressDeviceStats.argtypes = [c.c_void_p]; L.LizardGPU_streamCompressDeviceStats.restype = c.c_int
    L.LizardGPU_decompressFrames_device.argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint,
                                                    c.c_void_p]
    L.LizardGPU_decompressFrames_device.restype = c.c_int
    L.LizardGPU_framesInfo_device.argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_framesInfo_device.restype = c.c_int
    L.LizardGPU_framesDecodeDeviceStats.argtypes = [c.c_void_p]; L.LizardGPU_framesDecodeDeviceStats.restype = c.c_int
    L.LizardGPU_decompressStream_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint,
                                                    c.c_void_p]
    L.LizardGPU_decompressStream_device.restype = c.c_size_t
    L.LizardGPU_streamIndex_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p,
                                               c.c_void_p, c.c_void_p]
    L.LizardGPU_streamIndex_device.restype = c.c_int
    L.LizardGPU_streamDecodeDeviceStats.argtypes = [c.c_void_p]; L.LizardGPU_streamDecodeDeviceStats.restype = c.c_int
    L.LizardGPU_splitPlanes_device.argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_splitPlanes_device.restype = c.c_int
    L.LizardGPU_joinPlanes_device.argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_joinPlanes_device.restype = c.c_int
    L.LizardGPU_planesStats.argtypes = [c.c_void_p]; L.LizardGPU_planesStats.restype = c.c_int
    for name in ("LizardGPU_splitBitPlanes_device", "LizardGPU_joinBitPlanes_device"):
        getattr(L, name).argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
        getattr(L, name).restype = c.c_int
    L.LizardGPU_bitPlanesStats.argtypes = [c.c_void_p]; L.LizardGPU_bitPlanesStats.restype = c.c_int
    L.LizardGPU_tensorHeaderWrite2.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p]; L.LizardGPU_tensorHeaderWrite2.restype = c.c_size_t
    L.LizardGPU_tensorHeaderRead2.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]; L.LizardGPU_tensorHeaderRead2.restype = c.c_int
    L.LizardGPU_tensorHeaderWrite.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p]; L.LizardGPU_tensorHeaderWrite.restype = c.c_size_t
    L.LizardGPU_tensorHeaderRead.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]; L.LizardGPU_tensorHeaderRead.restype = c.c_int
    for name in ("LizardGPU_splitPlanesXor_device", "LizardGPU_joinPlanesXor_device"):
        getattr(L, name).argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint, c.c_void_p]
        getattr(L, name).restype = c.c_int
    L.LizardGPU_planesXorStats.argtypes = [c.c_void_p]; L.LizardGPU_planesXorStats.restype = c.c_int
    L.LizardGPU_tensorHeaderWrite3.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p]; L.LizardGPU_tensorHeaderWrite3.restype = c.c_size_t
    L.LizardGPU_tensorHeaderRead3.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]; L.LizardGPU_tensorHeaderRead3.restype = c.c_int
    L.LizardGPU_seekTableBytes.argtypes = [c.c_size_t]; L.LizardGPU_seekTableBytes.restype = c.c_size_t
    L.LizardGPU_seekTableWrite.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t]; L.LizardGPU_seekTableWrite.restype = c.c_size_t
    L.LizardGPU_seekTableRead.argtypes = [c.c_void_p, c.c_size_t, c.c_uint64, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    L.LizardGPU_seekTableRead.restype = c.c_int
    L.LizardGPU_compressSeekableStream_device.argtypes = L.LizardGPU_compressStream_device.argtypes
    L.LizardGPU_compressSeekableStream_device.restype = c.c_size_t
    L.LizardGPU_seekTable_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_seekTable_device.restype = c.c_int
    L.LizardGPU_decompressSeekableStream_device.argtypes = L.LizardGPU_decompressStream_device.argtypes
    L.LizardGPU_decompressSeekableStream_device.restype = c.c_size_t
    L.LizardGPU_decompressStreamItems_device.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p,
                                                         c.c_uint, c.c_void_p]
    L.LizardGPU_decompressStreamItems_device.restype = c.c_size_t
    L.LizardGPU_seekDeviceStats.argtypes = [c.c_void_p]; L.LizardGPU_seekDeviceStats.restype = c.c_int
    L.LizardGPU_planesRangeBytes.argtypes = [c.c_uint64, c.c_uint32, c.c_uint32, c.c_uint64, c.c_uint64, c.c_void_p, c.c_size_t]
    L.LizardGPU_planesRangeBytes.restype = c.c_size_t
    L.LizardGPU_frameRangesBound.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t]; L.LizardGPU_frameRangesBound.restype = c.c_size_t
    L.LizardGPU_decompressFrameRanges_device.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.LizardGPU_decompressFrameRanges_device.restype = c.c_int
    L.LizardGPU_sliceDeviceStats.argtypes = [c.c_void_p]; L.LizardGPU_sliceDeviceStats.restype = c.c_int
    L.LizardGPU_joinPlanesRange_device.argtypes = [c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]; L.LizardGPU_joinPlanesRange_device.restype = c.c_int
    _lib = L
    return L


_ERR = {1: "no HIP device", 2: "level not implemented on the GPU path", 3: "bad argument", 4: "HIP call failed",
        5: "out of memory", 6: "RCCL failure"}


def check(rc, what):
    if rc < 0:
        detail = lib().LizardGPU_lastError().decode(errors="replace")
        raise LizardAmdError(f"{what}: {_ERR.get(-rc, rc)} {detail}".strip())
    return rc


def check_frame(code, what):
    """A size_t result of the frame entries: the value, or LizardAmdError with the reference's error name."""
    L = lib()
    if L.LizardGPU_frameIsError(code):
        name = L.LizardF_getErrorName(code).decode()
        detail = L.LizardGPU_lastError().decode(errors="replace")
        raise LizardAmdError(f"{what}: {name} {detail}".strip())
    return code
