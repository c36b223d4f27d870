"""Exact MPE on the junction tree as a host walk of the planner's item tables, stand-alone on a CPU: tests/cpp/test_jt_mpe_walk.cpp
is compiled together with bayesiannetwork_amd/csrc/bn_jt_plan.cpp alone and run as a program of its own, once plainly and once under
AddressSanitizer and UndefinedBehaviorSanitizer.  It does collect, pick, distribute, read-out and states the way jt_mpe_kernel
indexes them, every index bounds-checked, against the enumeration of the joint: Pearl's network, the two-node tie network and a
3 x 3 grid."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_walk_of_the_item_tables(tmp_path, sanitize):
    exe = str(tmp_path / "test_jt_mpe_walk")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_jt_mpe_walk.cpp"),
           os.path.join(CSRC, "bn_jt_plan.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
