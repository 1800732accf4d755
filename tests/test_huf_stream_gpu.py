"""GPU: lz_put_stream_huf (lizard_amd/csrc/lz_huf.h) alone on the device over the named streams of tests/huf_stream_inputs.py — the
streams tests/test_huf_stream_emul.py shows to reach every path of the stage — against the oracle's bytes, through the product's own
wave primitives, which the emulator replaces: tests/huf_stream_kernels.hip, one run of the program for the whole set."""
import os
import re
import subprocess

import pytest

import huf_stream_inputs as H
import util

pytestmark = pytest.mark.gpu


def test_huf_stage_on_the_device_stream_by_stream(tmp_path):
    """Every stream in three forms — alone in a wave at every residue of its source and output address, eight in a row through one
    workspace, and in pairs through a pool of three workspaces that the 8 waves of a workgroup share — gives the expected bytes and
    the expected `huffed` flag, and changes nothing outside its n + 3 output bytes."""
    exe = os.path.join(util.ROOT, "tests", "huf_stream_kernels")
    assert os.path.exists(exe), "tests/huf_stream_kernels is built by __graft_entry__.build()"
    cases = str(tmp_path / "huf_streams.bin")
    n = H.write_case_file(cases)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0 and " mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"cases: (\d+) mismatches: 0", r.stdout)
    assert m and int(m.group(1)) == 3 * n, (r.stdout, n)
