"""bn::learning::greedy / k2_algorithm of the C++ drop-in (include/bayesian/learning/, compiled over include/compat like
tests/cpp/test_scores.cpp): the device path (Eval = aic / mdl) against the reference's literal loop in the same binary (a trivial
subclass of aic / mdl forces it; same seed, so the same shuffles) -- equal edges -- and against the Python learner fed the
visits the binary prints -- equal edges and a bit-equal score.  Before edges are compared, the margin condition of the header's
contract is asserted on exactly the visits the binary made (libm restatement, tests/learning_refs.py)."""
import json
import os
import subprocess

import pytest

import learning_refs as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_learning.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
ALARM = os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc")


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_learning")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           SRC, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_cpp_learners_equal_the_literal_loop_and_the_python_learner(bnlib, tmp_path):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner
    model, table, _, _, _ = LR.learning_input("alarm2k_mdl")
    path = tmp_path / "samples.txt"
    path.write_text("".join(f"{int(c)} " + " ".join(str(int(s)) for s in row) + "\n" for row, c in zip(table.pats, table.counts)))
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe, ALARM, str(path), "12345"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    assert d["n"] == model.n and d["greedy_aic_cpts_ok"] is True
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        for name, criterion in (("greedy_aic", "aic"), ("k2_mdl", "mdl"), ("hint_mdl", "mdl")):
            dev, lit = d[name], d[name + "_literal"]
            assert dev["visits"] == lit["visits"] and len(dev["visits"]) > 0, name        # the same seed: the same shuffles
            # the margin condition on these very visits, before any decision is compared
            ref = LR.RefLearner(model.k, LR.empty_graph(model.n), criterion, table.total, table.libm_ll, record=True)
            for child, cand in dev["visits"]:
                ref.try_parents(child, cand)
            ms = LR.margins(table, ref)
            print(f"{name}: {len(ms)} decisions, {len(dev['edges'])} edges, smallest margin / bound {min(m / b for m, b in ms):.3g}")
            assert all(m > 1000 * b for m, b in ms), name
            assert sorted(map(tuple, dev["edges"])) == sorted(map(tuple, lit["edges"])) == [tuple(e) for e in sorted(
                (u, v) for v, ps in enumerate(ref.parents) for u in ps)], name
            assert len(dev["edges"]) > 0
            assert abs(dev["score"] - lit["score"]) <= LR.graph_bound(table, ref.parents, criterion), name
            with Learner(t, None, criterion) as L:
                for child, cand in dev["visits"]:
                    L.try_parents(child, cand)
                assert sorted((u, v) for v, ps in enumerate(L.parents()) for u in ps) == sorted(map(tuple, dev["edges"])), name
                assert L.score() == dev["score"], name                                     # bit for bit: a function of the counts
    k2 = d["k2_mdl"]
    assert all(e[0] not in (0, 1, 2) for e in k2["edges"] if e[1] == 3)                    # the precondition held
    assert all(e[0] >= model.n // 2 for e in k2["edges"] if e[1] == model.n - 1)
    hint = d["hint_mdl"]
    assert all(u < model.n // 2 <= v for u, v in hint["edges"])
