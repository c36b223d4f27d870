"""Which kernel runs a query (bayesiannetwork_amd/csrc/bn_engine_policy.cpp: the resident launch shape for a CU count, the 0.9 x CUs
caps, and the predicates that choose between the one-launch paths) checked stand-alone on a CPU: tests/cpp/test_engine_policy.cpp is
compiled together with the policy file alone under AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own.
It writes the facts by hand, so both sides of every threshold are reached -- on 64, 256 and 304 CUs -- without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


def test_path_choice_on_both_sides_of_every_threshold(tmp_path):
    exe = str(tmp_path / "test_engine_policy")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_engine_policy.cpp"), os.path.join(CSRC, "bn_engine_policy.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
