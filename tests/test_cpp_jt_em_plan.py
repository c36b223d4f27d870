"""The family tables of exact expectation-maximisation and the rows of one of its launches, stand-alone on a CPU:
tests/cpp/test_jt_em_plan.cpp is compiled together with bayesiannetwork_amd/csrc/bn_jt_plan.cpp and bn_engine_policy.cpp alone and run
as a program of its own, once plainly and once under AddressSanitizer and UndefinedBehaviorSanitizer.  It walks the family tables the
way jt_em_kernel indexes them, every index bounds-checked, against the enumeration of the joint on Pearl's network and a 3 x 3 grid,
and checks bn_policy::jt_em_plan on both sides of each of its limits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_walk_of_the_family_tables_and_rows_per_launch(tmp_path, sanitize):
    exe = str(tmp_path / "test_jt_em_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_jt_em_plan.cpp"),
           os.path.join(CSRC, "bn_jt_plan.cpp"), os.path.join(CSRC, "bn_engine_policy.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
