"""bn::learning::junction_tree_em (include/bayesian/learning/junction_tree_em.hpp), the C++ face of bn_jt_em_fit:
tests/cpp/test_jt_em.cpp is compiled by plain g++ against the stand-in data model of include/compat and the in-tree library and run on
the GPU -- Pearl's structure, a table with unobserved cells: the fitted tables land in the vertices' cpt, a complete table gives the
relative frequencies, malformed arguments throw -- and what it prints equals Engine.jt_em_fit and the host restatement bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_jt_em.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_jt_em")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"), SRC,
           "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_junction_tree_em_header_compiles(bnlib, tmp_path):
    build(tmp_path)


@pytest.mark.gpu
def test_junction_tree_em_functor_on_pearl(bnlib, tmp_path):
    import jtem_refs
    from bayesiannetwork_amd import from_parent_lists
    from bayesiannetwork_amd.engine import Engine
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["failures"] == 0
    model = from_parent_lists([2, 2, 2, 2], [[], [], [0], [0, 1]],
                              [[0.3, 0.7], [0.4, 0.6], [0.9, 0.1, 0.2, 0.8], [0.7, 0.3, 0.6, 0.4, 0.8, 0.2, 0.1, 0.9]], name="pearl_positive")
    M = 255
    pats = np.asarray([[0, 1, M, 0], [1, M, 1, 1], [M, M, M, M], [1, 0, 0, M], [0, 0, 1, 1], [M, 1, M, 0], [1, 1, 1, 0], [M, 0, M, 1]], np.uint8)
    counts = np.asarray([5, 3, 2, 7, 1, 4, 6, 2], np.uint64)
    with Engine(model, device=0) as eng:
        plan = eng.jt_plan()
        cpt, iters, hist, lls = eng.jt_em_fit(pats, counts, max_iters=5, tol=0.0)
        sixth, _, _, _ = eng.jt_em_fit(pats, counts, max_iters=1, tol=0.0, cpt_init=cpt)
        assert eng.info("jt_em_skipped") == 0
    assert d["iters"] == iters == 5 and d["skipped"] == 0
    assert np.array_equal(np.asarray(d["cpt"]), cpt)            # (%.17g round-trips a double)
    assert np.array_equal(np.asarray(d["deltas"]), hist)
    assert np.array_equal(np.asarray(d["logliks"]), lls)
    assert np.array_equal(np.asarray(d["sixth"]), sixth)
    want = jtem_refs.em_fit(model, plan, pats, counts, max_iters=6, tol=0.0)
    assert np.array_equal(cpt, want["thetas"][4]) and np.array_equal(sixth, want["thetas"][5])
