"""How an EM E-step's pattern rows are cut into launches, and where the 256-blocks of the expected-count sum close (bn_policy::em_plan /
em_chunk in bayesiannetwork_amd/csrc/bn_engine_policy.cpp), checked stand-alone on a CPU: tests/cpp/test_em_plan.cpp is compiled together
with the policy file alone and run as a program of its own, once plainly and once under AddressSanitizer and UndefinedBehaviorSanitizer.
It sets the scratch limit to a few hundred cells so that launch edges fall inside a block, and checks that every cut closes the same
blocks with the same rows in the same order."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_em_chunks_and_block_sums(tmp_path, sanitize):
    exe = str(tmp_path / "test_em_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_em_plan.cpp"),
           os.path.join(CSRC, "bn_engine_policy.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
