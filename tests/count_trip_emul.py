"""TEST INFRASTRUCTURE ONLY: builds and drives tests/emul/count_trip_api.cpp (the split form of levels 10 / 30 on the SIMT emulator
with the count-trip and check-bit marks counted), one library per setting of the switches."""
import ctypes
import os
import subprocess

import util

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
CSRC = os.path.join(util.ROOT, "lizard_amd", "csrc")
MARKS = 10


def lib(late=None, check_lo=None):
    """tests/emul/libcount_trip_*.so from simt.cpp + count_trip_api.cpp; None = the tree's default for that switch."""
    defs = ["-D%s=%d" % (k, v) for k, v in (("LZ_BACK_LATE", late), ("LZ_CHECK_LO", check_lo)) if v is not None]
    tag = "".join(d[5:].replace("=", "").lower() for d in defs) or "default"
    out = os.path.join(EMUL, "libcount_trip_%s.so" % tag)
    srcs = [os.path.join(EMUL, "simt.cpp"), os.path.join(EMUL, "count_trip_api.cpp")]
    deps = srcs + [os.path.join(EMUL, "lz_wave.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in deps):
        tmp = "%s.tmp.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                               "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-I", EMUL, "-o", tmp] + defs + srcs)
        os.replace(tmp, out)
    L = ctypes.CDLL(out)
    L.emul_ct_split.restype = ctypes.c_int
    L.emul_ct_split.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    return L


def knobs(L):
    k = (ctypes.c_uint * 2)()
    L.emul_ct_knobs(k)
    return tuple(int(x) for x in k)


def marks(L, reset=True):
    out = (ctypes.c_ulonglong * 16)()
    L.emul_ct_marks(out, 1 if reset else 0)
    return {k: int(out[k]) for k in range(MARKS)}


def run(L, area, blocks, level, nprod=1, ncons=1, lane_forms=-1, seed=1):
    """The batch `blocks` = [(offset, size)] of `area`; returns the outputs."""
    nb = len(blocks)
    src = ctypes.create_string_buffer(bytes(area), len(area))
    offs = (ctypes.c_ulonglong * nb)(*[o for o, _ in blocks])
    sizes_in = (ctypes.c_uint * nb)(*[n for _, n in blocks])
    stride = util.oracle().lzo_compress_bound(max(n for _, n in blocks)) + 64
    dst = ctypes.create_string_buffer(nb * stride)
    sizes = (ctypes.c_uint * nb)()
    assert L.emul_ct_split(src, nb, offs, sizes_in, dst, stride, sizes, level, nprod, ncons, lane_forms, seed) == 0
    return [dst.raw[i * stride:i * stride + sizes[i]] for i in range(nb)]
