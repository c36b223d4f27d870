"""bn::inference::junction_tree::mpe (include/bayesian/inference/junction_tree.hpp), the C++ face of bn_jt_mpe_run:
tests/cpp/test_junction_tree_mpe.cpp is compiled by plain g++ against the stand-in data model of include/compat and the in-tree
library and run on the GPU -- Pearl's network with H = 0: the decoded assignment is the enumeration's argmax, the log probability
log of the best joint, an mpe() call between two operator() calls changes nothing -- and what it prints equals the Python result
exactly."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_junction_tree_mpe.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_junction_tree_mpe")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"), SRC,
           "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_junction_tree_mpe_compiles(bnlib, tmp_path):
    build(tmp_path)


@pytest.mark.gpu
def test_junction_tree_mpe_on_pearl(bnlib, tmp_path):
    from bayesiannetwork_amd import Evidence, synth
    from bayesiannetwork_amd.engine import Engine
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["failures"] == 0
    model = synth.pearl()
    with Engine(model, device=0) as e:
        got = e.jt_mpe_run(Evidence.from_dict(model, {3: 0}))
    assert d["states"] == got["states"].tolist()
    assert np.array_equal(np.asarray(d["max_marginals"]), got["max_marginals"])   # (%.17g round-trips a double)
    assert d["log_p"] == got["log_p"]
