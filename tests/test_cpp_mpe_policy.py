"""Which form of the max-product kernels runs a network (bn_policy::mpe_form in bayesiannetwork_amd/csrc/bn_engine_policy.cpp) checked
stand-alone on a CPU: tests/cpp/test_mpe_policy.cpp is compiled together with the policy file alone and run as a program of its own,
once plainly and once under AddressSanitizer and UndefinedBehaviorSanitizer.  It writes the facts by hand -- small plan ok / not ok, the
several-workgroup plan on both sides of 0.9 x CUs at 64, 256 and 304 CUs, forced forms -- without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_mpe_form_on_both_sides_of_every_threshold(tmp_path, sanitize):
    exe = str(tmp_path / "test_mpe_policy")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_mpe_policy.cpp"),
           os.path.join(CSRC, "bn_engine_policy.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
