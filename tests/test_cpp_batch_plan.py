"""How a batch of evidence sets is planned (bayesiannetwork_amd/csrc/bn_engine_policy.cpp: the four batch predicates with the
900-tile threshold, the rule that sends a batch to the second, dense engine and the same-bits rule that refuses it, the chunks of
the resident, the several-workgroup and the DAG path; bn_batch_stage.cpp: the layout of the evidence staging block) checked
stand-alone on a CPU: tests/cpp/test_batch_plan.cpp is compiled together with those two files alone under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


def test_batch_policy_chunks_and_staging_layout(tmp_path):
    exe = str(tmp_path / "test_batch_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_batch_plan.cpp"), os.path.join(CSRC, "bn_engine_policy.cpp"),
           os.path.join(CSRC, "bn_batch_stage.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
