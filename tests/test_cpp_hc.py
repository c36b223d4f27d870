"""bn::learning::stepwise_structure_hc of the C++ drop-in (include/bayesian/learning/stepwise_structure_hc.hpp, compiled over
include/compat like tests/cpp/test_anneal.cpp): the device path (Eval = aic, BetweenLearning = greedy: 64 resident runs) and the
host path (a trivial subclass of aic forces the literal loop, one run) each return a DAG; operator()'s return equals the aic functor
of the returned graph within learning_refs.graph_bound; the device path equals the Python learner with the same seed -- equal
edges and a bit-equal score.  Both leave edges only from a merge's parent cluster to its child cluster: the host path's
learn_with_hint calls (a recording BetweenLearning) are, in order and node for node, the plan hc_refs.cluster_plan replays from
the device's mutual information and run 0's stream -- so a swapped coin or a wrong id order shows -- and every edge runs from the
parent list to the child list of one call; the device path's edges are held to the winner's merge trace.  mutual_information_holder answers from one all-pairs call what the functors answer pair by pair."""
import json
import os
import subprocess

import pytest

import hc_refs as HR
import learning_refs as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hc.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
ALARM = os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc")
SEED, ALPHA = 77, 0.3


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_hc")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           SRC, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def is_dag(n, edges):
    parents = [[] for _ in range(n)]
    for u, v in edges:
        parents[v].append(u)
    left, order = [len(p) for p in parents], [v for v in range(n) if not parents[v]]
    for u in order:
        for v in range(n):
            if u in parents[v]:
                left[v] -= 1
                if left[v] == 0:
                    order.append(v)
    return len(order) == n, parents


def test_cpp_hc_both_paths_and_the_python_learner(bnlib, tmp_path):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable
    model, table, _, _, _ = LR.learning_input("alarm2k_aic")
    path = tmp_path / "samples.txt"
    path.write_text("".join(f"{int(c)} " + " ".join(str(int(s)) for s in row) + "\n" for row, c in zip(table.pats, table.counts)))
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe, ALARM, str(path), str(SEED), repr(ALPHA)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    assert d["n"] == model.n and d["negative_alpha_refused"] is True
    for name in ("device", "host"):
        run = d[name]
        ok, parents = is_dag(model.n, run["edges"])
        assert ok and len(run["edges"]) > 0, name
        assert abs(run["score"] - run["aic"]) <= LR.graph_bound(table, parents, "aic"), name
    assert all(sum(1 for e in d["device"]["edges"] if e[1] == v) <= 3 for v in range(model.n))
    assert d["holder_mi"] == pytest.approx(d["functor_mi"], abs=1e-12) and d["holder_h"] == pytest.approx(d["functor_h"], abs=1e-12)
    with InfoTable(table.pats, table.counts, model.k, device=0) as t, TermTable(t, 3) as tt, Learner(t, None, "aic") as L:
        rec = L.hc(tt, ALPHA, 64, SEED)
        assert sorted((u, v) for v, ps in enumerate(L.parents()) for u in ps) == sorted(map(tuple, d["device"]["edges"]))
        assert L.score() == d["device"]["score"] and rec["winner"] == d["winner"]                     # bit for bit
        # the host path: the calls are the plan, and every edge runs from a call's parent list to its child list
        exponents = []
        calls, decisions = HR.cluster_plan(t.pair_entropies()["mi"], model.n, ALPHA, SEED, 0, exponents)
        assert HR.pow_margin_ok(decisions, ALPHA, exponents), "a pruning decision within 2^-40 of its threshold: change SEED"
        assert [(list(p), list(c)) for p, c in d["hint_calls"]] == calls and len(calls) > 1
        assert any(len(p) > 1 for p, _ in calls) and any(len(c) > 1 for _, c in calls)
        for u, v in d["host"]["edges"]:
            assert any(u in p and v in c for p, c in calls), (u, v)
        # the device path: the winner's merges, from its trace
        traced = L.hc(tt, ALPHA, 64, SEED, trace_run=rec["winner"])
        nodes = {i: [i] for i in range(model.n)}
        merges = []
        for s, m in enumerate(traced["merge_trace"]):
            merges.append((nodes[int(m.parent)], nodes[int(m.child)]))
            nodes[model.n + s] = nodes[int(m.parent)] + nodes[int(m.child)]
        assert len(merges) == int(traced["merges"][rec["winner"]]) > 1
        for u, v in d["device"]["edges"]:
            assert any(u in p and v in c for p, c in merges), (u, v)
