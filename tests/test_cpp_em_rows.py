"""The M-step's row array (bn_policy::em_rows in bayesiannetwork_amd/csrc/bn_engine_policy.cpp: per CPT entry the first entry of its row
and the node's arity), checked stand-alone on a CPU: tests/cpp/test_em_rows.cpp is compiled together with the policy file alone and run
as a program of its own, once plainly and once under AddressSanitizer and UndefinedBehaviorSanitizer.  Its cases: roots of arity 1 and
2, a node with parents of arities 2 and 3 and own arity 4, mixed arities back to back, and an entry beyond 65 535."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_em_rows(tmp_path, sanitize):
    exe = str(tmp_path / "test_em_rows")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_em_rows.cpp"),
           os.path.join(CSRC, "bn_engine_policy.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())
