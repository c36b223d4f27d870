"""bn::learning::hill_climbing of the C++ drop-in (include/bayesian/learning/hill_climbing.hpp, compiled over include/compat like
tests/cpp/test_anneal.cpp): the functor's result equals bn_learn_climb's through the Python learner on the same table and seed --
equal edges and a bit-equal score -- as the classic greedy climb under mdl, aic and bdeu, and as a tabu search with perturbed
restarts under mdl, where the winning run agrees too."""
import json
import os
import subprocess

import pytest

import learning_refs as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hill_climbing.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
ALARM = os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc")
SEED, TABU_LEN, MAX_WORSE, PERTURB, RUNS, MAX_STEPS = 99, 8, 6, 12, 9, 150


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_hill_climbing")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           SRC, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_cpp_hill_climbing_equals_the_python_learner(bnlib, tmp_path):
    from bayesiannetwork_amd.evaluation import BDeu, InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable
    model, table, _, _, _ = LR.learning_input("alarm2k_mdl")
    path = tmp_path / "samples.txt"
    path.write_text("".join(f"{int(c)} " + " ".join(str(int(s)) for s in row) + "\n" for row, c in zip(table.pats, table.counts)))
    exe = build_cpp(tmp_path)
    args = [str(x) for x in (SEED, TABU_LEN, MAX_WORSE, PERTURB, RUNS, MAX_STEPS)]
    out = subprocess.run([exe, ALARM, str(path)] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    assert d["n"] == model.n and d["tabu_65_refused"] is True and d["other_eval_refused"] is True
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        for name, crit in (("greedy_mdl", "mdl"), ("greedy_aic", "aic"), ("greedy_bdeu", BDeu(1.0))):
            with TermTable(t, 3, crit) as tt, Learner(t, None, crit) as L:
                empty = L.score()
                L.climb(tt, max_steps=MAX_STEPS)
                assert sorted((u, v) for v, ps in enumerate(L.parents()) for u in ps) == sorted(map(tuple, d[name]["edges"])), name
                assert L.score() == d[name]["score"] < empty and len(d[name]["edges"]) > 0, name                # bit for bit
        with TermTable(t, 3, "mdl") as tt, Learner(t, None, "mdl") as L:
            rec = L.climb(tt, TABU_LEN, MAX_WORSE, RUNS, PERTURB, SEED, max_steps=MAX_STEPS)
            assert sorted((u, v) for v, ps in enumerate(L.parents()) for u in ps) == sorted(map(tuple, d["tabu_mdl"]["edges"]))
            assert L.score() == d["tabu_mdl"]["score"] and rec["winner"] == d["winner"]
        assert all(sum(1 for e in d["tabu_mdl"]["edges"] if e[1] == v) <= 3 for v in range(model.n))
