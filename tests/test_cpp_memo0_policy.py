"""The host decisions of the resident path's first-sweep image (bayesiannetwork_amd/csrc/bn_engine_policy.cpp memo0_*: whether a run
starts from the image, which nodes go back to "no evidence" when a set replaces another, the part of sweep 0's residual the nodes
without evidence contribute) checked stand-alone on a CPU: tests/cpp/test_memo0_policy.cpp is compiled together with the policy file
alone under AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


def test_memo0_decisions(tmp_path):
    exe = str(tmp_path / "test_memo0_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_memo0_policy.cpp"), os.path.join(CSRC, "bn_engine_policy.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
