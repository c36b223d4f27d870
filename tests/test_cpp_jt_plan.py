"""The junction-tree planner (bayesiannetwork_amd/csrc/bn_jt_plan.cpp) checked stand-alone on a CPU: tests/cpp/test_jt_plan.cpp is
compiled together with the planner alone and run as a program of its own, once plainly and once under AddressSanitizer and
UndefinedBehaviorSanitizer.  It checks the tree's properties and walks the item tables as the kernel does, every index bounds-checked,
against the enumeration of the joint: one node, two unconnected nodes, a chain, a collider, a 3 x 3 grid, a 13-variable clique, the
scratch budget at exactly the plan's size and one cell below it, a clique of exactly 2^20 entries and the next size up."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_planner_tables_and_limits(tmp_path, sanitize):
    exe = str(tmp_path / "test_jt_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_jt_plan.cpp"),
           os.path.join(CSRC, "bn_jt_plan.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
