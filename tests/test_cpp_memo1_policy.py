"""The host decisions of the resident path's second-sweep image (bayesiannetwork_amd/csrc/bn_engine_policy.cpp memo1_*: whether a run
starts at sweep 2, the node-level adjacency, the seed of sweep 1's residual, the work limit and the image's own list of what it holds
across a set that does not patch) checked stand-alone on a CPU: tests/cpp/test_memo1_policy.cpp is compiled together with the policy
file alone under AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


def test_memo1_decisions(tmp_path):
    exe = str(tmp_path / "test_memo1_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_memo1_policy.cpp"), os.path.join(CSRC, "bn_engine_policy.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
