"""bn::learning::simulated_annealing of the C++ drop-in (include/bayesian/learning/simulated_annealing.hpp, compiled over
include/compat like tests/cpp/test_learning.cpp): the device path with one chain against the reference's literal loop on the host
in the same binary (a trivial subclass of mdl forces it; same seed, chain 0 of the same stream) -- equal edges, once every uphill
decision of the literal run has passed the exp-margin condition of tests/anneal_refs.py -- and the default 64 chains against the
Python learner with the same seed -- equal edges and a bit-equal score."""
import json
import os
import subprocess

import numpy as np
import pytest

import anneal_refs as AR
import learning_refs as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_anneal.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
ALARM = os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc")
SEED, T0, T1, RATE = 4321, 5.0, 0.5, 0.9   # 22 operated proposals per chain


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_anneal")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           SRC, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_cpp_annealing_equals_the_literal_loop_and_the_python_learner(bnlib, tmp_path):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable
    model, table, _, _, _ = LR.learning_input("alarm2k_mdl")
    path = tmp_path / "samples.txt"
    path.write_text("".join(f"{int(c)} " + " ".join(str(int(s)) for s in row) + "\n" for row, c in zip(table.pats, table.counts)))
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe, ALARM, str(path), str(SEED), repr(T0), repr(T1), repr(RATE)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    assert d["n"] == model.n and d["rate_one_refused"] is True
    # the margin condition on every uphill decision of the literal run, before any edge is compared
    assert len(d["uphill"]) > 0 and AR.exp_margin_ok([tuple(x) for x in d["uphill"]])
    one, lit = d["one_chain"], d["literal"]
    assert sorted(map(tuple, one["edges"])) == sorted(map(tuple, lit["edges"])) and len(one["edges"]) > 0
    parents = [[] for _ in range(model.n)]
    for u, v in one["edges"]:
        parents[v].append(u)
    assert abs(one["score"] - lit["score"]) <= LR.graph_bound(table, parents, "mdl")
    with InfoTable(table.pats, table.counts, model.k, device=0) as t, TermTable(t, 3) as tt:
        for run, chains in ((one, 1), (d["chains64"], 64)):
            with Learner(t, None, "mdl") as L:
                rec = L.anneal(tt, T0, T1, RATE, chains=chains, seed=SEED, rule="metropolis")
                assert sorted((u, v) for v, ps in enumerate(L.parents()) for u in ps) == sorted(map(tuple, run["edges"])), chains
                assert L.score() == run["score"], chains                                      # bit for bit
                assert chains == 1 or rec["winner"] == d["winner"]
        assert all(sum(1 for e in d["chains64"]["edges"] if e[1] == v) <= 3 for v in range(model.n))
        assert d["chains64"]["score"] <= one["score"]
