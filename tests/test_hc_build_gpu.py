"""GPU: the chain build of the hashChain / noChain levels (lz_hc_build, lz_hc_hits_plain, lz_hc_hits of lizard_amd/csrc/lz_hashchain.h)
alone on the device over the named inputs of tests/hc_build_inputs.py — the inputs tests/test_hc_build_emul.py shows to reach every
marked path of the build — table by table against the sequential model of the oracle, on the product's own DS atomics and region
pool, which the emulator replaces: tests/hc_build_kernels.hip, one run of the program for the whole set."""
import os
import re
import subprocess

import pytest

import hc_build_inputs as H
import util

pytestmark = pytest.mark.gpu


def test_chain_build_on_the_device_table_by_table(tmp_path):
    """Every input and variant in three forms — alone in a workgroup, sixteen in a workgroup whose waves queue for three chain-build
    regions, eight in a row through one wave's slot — gives the model's prev, chain2 and hit bits at every position, a best[] that is
    open only where the model allows it and the model's first search everywhere else, and changes nothing outside its slot."""
    exe = os.path.join(util.ROOT, "tests", "hc_build_kernels")
    assert os.path.exists(exe), "tests/hc_build_kernels is built by __graft_entry__.build()"
    cases = str(tmp_path / "hc_build_cases.bin")
    n = H.write_case_file(cases)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0 and " mismatches: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
    m = re.search(r"cases: (\d+) mismatches: 0", r.stdout)
    assert m and int(m.group(1)) == 3 * n, (r.stdout, n)
