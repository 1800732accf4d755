"""The compress kernels' memory footprint on the CPU: the kernel bodies of lizard_amd/csrc on the SIMT emulator, as a program of
its own under AddressSanitizer and UndefinedBehaviorSanitizer (tests/emul_asan_main.cpp).

tests/emul/emul_api.cpp is compiled with -DLZ_EMUL_EXACT_AREAS for it: every area a kernel is handed — hash table, tag array /
Slice::ws, Huffman workspace, occupancy summary, chain-build region, hashChain work area, sequence ring, scratch slot, and the
split form's arena, shared words, tables, rings and workspaces — is a heap allocation of exactly the size lz_kernels.h and
lizard_gpu.hip give it, with the template arguments of the kernel that serves the level.  Sources are malloc(n), destinations
malloc(Lizard_compressBound(n)) (the split form: slots of exactly the bound), the huff0 stage alone writes into n + 3 bytes.  A read
past a source, a store past the bound or past one of the kernel's own areas ends the program with a report; every output is
compared with the oracle compiled into the same program.  Nothing is loaded into python and no sanitizer runtime is preloaded.

Cases: all 23 levels x 17 sizes from 1 to 4 097 x seeds 0-3 x four kinds of data; one level per kernel family with and without
huff0 x 65 535 .. 262 145 x one seed per table form x the four kinds; levels 10 / 30 in the producer / consumer form with 1+1, 3+2
and 13+3 waves; the 301 named huff0 streams.

Measured on the CPU box (8 cores): 7 205 cases in 64 s on their own after 50 s of compiling (the five objects side by side); 90 s for
the test inside the whole suite.
"""
import functools
import os
import re
import subprocess

import pytest

import huf_stream_inputs
import util

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
CXX = ["-std=c++17", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread"]


def _build(out_dir):
    """The program, every source with the sanitizers; the five objects compile side by side."""
    emul = os.path.join(HERE, "emul")
    jobs = [
        (["gcc", "-std=gnu99"], os.path.join(util.ORACLE_DIR, "lizard_oracle.c")),
        (["gcc", "-std=gnu99"], os.path.join(util.ORACLE_DIR, "huf_oracle.c")),
        (["g++"] + CXX + ["-I", emul], os.path.join(emul, "simt.cpp")),
        (["g++"] + CXX + ["-I", emul, "-DLZ_EMUL_EXACT_AREAS"], os.path.join(emul, "emul_api.cpp")),
        (["g++"] + CXX, os.path.join(HERE, "emul_asan_main.cpp")),
    ]
    procs, objs = [], []
    for cmd, src in jobs:
        obj = os.path.join(out_dir, os.path.basename(src) + ".o")
        objs.append(obj)
        procs.append(subprocess.Popen(cmd + SAN + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate()[0] for p in procs]
    for p, log in zip(procs, logs):
        if p.returncode:
            raise subprocess.CalledProcessError(p.returncode, p.args, log)
    exe = os.path.join(out_dir, "emul_asan_main")
    subprocess.run(["g++"] + SAN + ["-pthread"] + objs + ["-o", exe], check=True, capture_output=True, text=True)
    return exe


@functools.lru_cache(maxsize=None)
def _sanitizer_runtime_present():
    """Can this compiler link a program with both sanitizers?  (A probe of one line, so that a failure to compile the real sources
    is never mistaken for a missing runtime.)"""
    r = subprocess.run(["g++", "-x", "c++", "-", "-fsanitize=address,undefined", "-o", os.devnull], input="int main() { return 0; }\n",
                       capture_output=True, text=True)
    return r.returncode == 0


def test_compress_kernels_under_address_sanitizer_with_exact_areas(tmp_path):
    """Exit status 0, a last line with a non-zero number of cases and `mismatches: 0`, and no sanitizer report."""
    if not _sanitizer_runtime_present():
        pytest.skip("no AddressSanitizer / UndefinedBehaviorSanitizer runtime")
    try:
        exe = _build(str(tmp_path))
    except subprocess.CalledProcessError as e:
        pytest.fail("the sanitized emulator program does not build:\n" + str(e.output or e.stderr)[-3000:])
    case_file = str(tmp_path / "huf_streams.bin")
    n_streams = huf_stream_inputs.write_case_file(case_file)
    r = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=1800, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    tail = (r.stdout + r.stderr)[-4000:]
    print(r.stdout[-400:])
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    last = r.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"cases: (\d+) mismatches: (\d+) seconds: [\d.]+", last)
    assert m, tail
    assert int(m.group(2)) == 0, tail
    # 14 family levels, their table forms, 6 sizes, 4 kinds; 23 levels x 17 sizes x 4 seeds x 4 kinds; 24 split runs; the streams
    forms = {10: 1, 30: 3, 11: 2, 31: 2, 12: 1, 33: 1, 13: 1, 34: 1, 20: 2, 40: 2, 21: 3, 41: 3, 22: 2, 42: 2}
    want = sum(forms.values()) * 6 * 4 + 23 * 17 * 4 * 4 + 24 + n_streams
    assert int(m.group(1)) == want, tail
