"""bn::inference::junction_tree (include/bayesian/inference/junction_tree.hpp), the C++ face of bn_jt_run: tests/cpp/test_junction_tree.cpp
is compiled by plain g++ against the stand-in data model of include/compat and the in-tree library and run on the GPU -- Pearl's
network with H = 0: the marginals equal the enumeration, operator() equals run() bit for bit, log_evidence() is log P(H = 0),
reload() sees an edited table -- and what it prints equals the Python result bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_junction_tree.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_junction_tree")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"), SRC,
           "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_junction_tree_header_compiles(bnlib, tmp_path):
    build(tmp_path)


@pytest.mark.gpu
def test_junction_tree_functor_on_pearl(bnlib, tmp_path):
    from bayesiannetwork_amd import Evidence, synth
    from bayesiannetwork_amd.engine import Engine
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["failures"] == 0
    model = synth.pearl()
    ev = Evidence.from_dict(model, {3: 0})
    with Engine(model, device=0) as e:
        got = e.jt_run(ev)
        assert np.array_equal(np.asarray(d["beliefs"]), got["beliefs"])   # (%.17g round-trips a double)
        assert d["log_evidence"] == got["log_evidence"]
        cpt = model.cpt.copy()
        lo = int(model.cpt_off[2])
        assert cpt[lo:lo + 2].tolist() == [1.0, 0.0]      # P(W | R = 0), the row the C++ test edits
        cpt[lo:lo + 2] = [0.0, 1.0]
        e.reload_cpt(cpt)
        assert np.array_equal(np.asarray(d["reloaded_beliefs"]), e.jt_run(ev)["beliefs"])
