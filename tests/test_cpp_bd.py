"""The Bayesian-Dirichlet scores of the C++ drop-in (include/bayesian/evaluation/bdeu.hpp under include/bayesian/learning/, compiled
over include/compat like tests/cpp/test_learning.cpp): greedy<bdeu>, k2_algorithm<k2_score> and simulated_annealing<bdeu> on the
device against their literal host twins in the same binary (a trivial subclass forces the literal loop; same seed, so the same
shuffles and the same stream), and against the Python learner fed the visits the binary prints.

The literal twins evaluate every candidate graph through the same device function the learner sums (evaluation::bdeu /
k2_score -> bn_learn_create_spec), in the same order: edges AND scores are demanded bit for bit, no margin is needed."""
import json
import os
import subprocess

import pytest

import anneal_refs as AR
import bd_refs as BD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_bd.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
SEED, T0, T1, RATE = 4321, 20.0, 0.5, 0.9


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_bd")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           SRC, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def nodes_only_dsc(k):
    """A network file with the nodes and arities alone (the binary drops the edges anyway)."""
    out = ['belief network "bd"']
    for v, kv in enumerate(k):
        states = ", ".join(f'"s{s}"' for s in range(int(kv)))
        out += [f"node V{v}", "{", f"  type: discrete[{int(kv)}] = {{ {states} }};", "}"]
    return "\n".join(out) + "\n"


def edges_of(parents):
    return sorted((u, v) for v, ps in enumerate(parents) for u in ps)


def test_cpp_bd_learners_equal_their_literal_twins_and_the_python_learner(bnlib, tmp_path):
    from bayesiannetwork_amd.evaluation import BDeu, InfoTable, K2Score
    from bayesiannetwork_amd.learning import Learner, TermTable
    model, table = BD.learner_input()
    (tmp_path / "net.dsc").write_text(nodes_only_dsc(model.k))
    (tmp_path / "samples.txt").write_text("".join(f"{int(c)} " + " ".join(str(int(s)) for s in row) + "\n"
                                                  for row, c in zip(table.pats, table.counts)))
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe, str(tmp_path / "net.dsc"), str(tmp_path / "samples.txt"), str(SEED), repr(T0), repr(T1), repr(RATE)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    assert d["n"] == model.n
    # the one step the two annealing runs do not share is exp: its margin on every uphill decision of the literal run, first
    assert len(d["uphill"]) > 0 and AR.exp_margin_ok([tuple(x) for x in d["uphill"]])
    for name in ("greedy_bdeu", "k2_k2", "anneal_bdeu"):
        dev, lit = d[name], d[name + "_literal"]
        assert dev["visits"] == lit["visits"], name
        assert sorted(map(tuple, dev["edges"])) == sorted(map(tuple, lit["edges"])) and len(dev["edges"]) > 0, name
        assert dev["score"] == lit["score"], name                                     # bit for bit: the same function
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        for name, crit in (("greedy_bdeu", BDeu()), ("k2_k2", K2Score())):
            with Learner(t, None, crit) as L:
                assert len(d[name]["visits"]) > 0
                for child, cand in d[name]["visits"]:
                    L.try_parents(child, cand)
                assert edges_of(L.parents()) == sorted(map(tuple, d[name]["edges"])) and L.score() == d[name]["score"], name
                if name == "greedy_bdeu":
                    parents = L.parents()
                    assert d["greedy_bdeu_eval"] == L.score()                          # evaluation::bdeu of the learned graph
                    assert d["greedy_bdeu_eval_ess"] == BDeu(2.5)(parents, t)          # basic_bdeu<std::ratio<5, 2>>
                    ll, _ = L.terms()
                    assert d["greedy_bdeu_eval_head"] == BD.likelihood_alone([ll[1], ll[0]])   # a vertex_list narrows and orders the sum
        with TermTable(t, 2, BDeu()) as tt:
            for name, chains in (("anneal_bdeu", 1), ("anneal_bdeu_16", 16)):
                with Learner(t, None, BDeu()) as L:
                    L.anneal(tt, T0, T1, RATE, chains=chains, seed=SEED, rule="metropolis")
                    assert edges_of(L.parents()) == sorted(map(tuple, d[name]["edges"])) and L.score() == d[name]["score"], name
            assert d["anneal_bdeu_16"]["score"] <= d["anneal_bdeu"]["score"]
            assert all(sum(1 for e in d["anneal_bdeu_16"]["edges"] if e[1] == v) <= 2 for v in range(model.n))
