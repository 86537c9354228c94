"""The unit and tile-class arithmetic of the hand-placed kernels, pinned on the CPU (no GPU).

csrc/hp_unit.h holds what fwd_hp_kernel, dq_hp_kernel and dkdv_hp_kernel share around their
generated statements; its first part -- HpRowUnit (b, hq, kv head, Lq, Lk, m0, ntiles) and the
tile classes of a wave (hp_n_full, hp_last_tile; live0 is last >= 0) -- is plain integer arithmetic
a host compiler takes.  tests/hp_unit_host_main.cpp, next to this file, includes the header and sweeps, causal and
not, Lq and Lk over 1 .. 400 (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 400 among them, Lq != Lk in
both directions), every row block and every wave, against a brute force over single rows and keys
with the visibility rule of DESIGN.md 2.  This test compiles it as host code and runs it.
"""
import os
import subprocess

import pytest

from fa2_triton_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "hp_unit_host_main.cpp")


@pytest.fixture(scope="module")
def compiler():
    try:
        return build.hipcc()
    except RuntimeError:
        pytest.skip("no hipcc to compile the host program with")


def test_unit_and_tile_classes_match_the_brute_force(compiler, tmp_path):
    exe = tmp_path / "hp_unit_host_main"
    cmd = [compiler, "-x", "c++", "-std=c++17", "-O1", "-g", "-I", build.CSRC, MAIN, "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    checks, mismatches = (int(x) for x in res.stdout.splitlines()[-1].split()[0:3:2])
    assert mismatches == 0 and checks > 20000, res.stdout


def test_host_part_names_no_hip():
    """What precedes the device part of hp_unit.h includes <stdint.h> only and names no HIP builtin."""
    text = open(os.path.join(build.CSRC, "hp_unit.h")).read()
    host = text[:text.index('#include "common.h"')]
    assert [ln.split()[1] for ln in host.splitlines() if ln.startswith("#include")] == ["<stdint.h>"]
    code = "\n".join(ln.split("//")[0] for ln in host.splitlines())
    assert "__builtin" not in code and "threadIdx" not in code and " min(" not in code and " max(" not in code
