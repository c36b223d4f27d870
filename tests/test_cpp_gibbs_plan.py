"""The planner of Gibbs sampling (bayesiannetwork_amd/csrc/bn_gibbs_plan.cpp) checked stand-alone on a CPU: tests/cpp/test_gibbs_plan.cpp
is compiled together with the planner alone and run as a program of its own, once plainly and once under AddressSanitizer and
UndefinedBehaviorSanitizer.  It checks that the colouring is proper and greedy and that every node is in exactly one slot, walks the
slot tables as the kernel does with every index bounds-checked, compares the child strides' rows with a direct computation, and
tries the limits on both sides (4096 / 4097 nodes, arities summing to 8192 / 8193) and the launch split below, at and above the cap."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_planner_tables_and_limits(tmp_path, sanitize):
    exe = str(tmp_path / "test_gibbs_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_gibbs_plan.cpp"),
           os.path.join(CSRC, "bn_gibbs_plan.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
