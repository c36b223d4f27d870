"""bn::learning::optimal_structure of the C++ drop-in (include/bayesian/learning/optimal_structure.hpp, compiled over include/compat
like tests/cpp/test_hill_climbing.cpp): the functor's result equals bn_learn_optimal's through the Python learner on the same table
-- equal edges, a bit-equal score and a bit-equal value -- under mdl, aic and bdeu, and under mdl with every node allowed its
lower-numbered nodes only."""
import json
import os
import subprocess

import pytest

import optimal_refs as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_optimal_structure.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
MAX_PARENTS = 3


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_optimal_structure")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           SRC, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def nodes_only_dsc(k):
    """A network description of nodes X0 .. with the given arities and no edges."""
    text = 'belief network "o13"\n'
    for v, kv in enumerate(k):
        states = ", ".join(f'"s{s}"' for s in range(int(kv)))
        text += f"node X{v}\n{{\n  type: discrete[{int(kv)}] = {{ {states} }};\n}}\n"
    return text


def test_cpp_optimal_structure_equals_the_python_learner(bnlib, tmp_path):
    from bayesiannetwork_amd.evaluation import BDeu, InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable
    model, table = OR.optimal_input("o13")
    net, path = tmp_path / "o13.dsc", tmp_path / "samples.txt"
    net.write_text(nodes_only_dsc(model.k))
    path.write_text("".join(f"{int(c)} " + " ".join(str(int(s)) for s in row) + "\n" for row, c in zip(table.pats, table.counts)))
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe, str(net), str(path), str(MAX_PARENTS)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    assert d["n"] == model.n and d["max_parents_0_refused"] is True and d["allowed_size_refused"] is True and d["other_eval_refused"] is True
    lower = [(1 << v) - 1 for v in range(model.n)]
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        for name, crit, allowed in (("mdl", "mdl", None), ("aic", "aic", None), ("bdeu", BDeu(1.0), None), ("mdl_lower", "mdl", lower)):
            with TermTable(t, MAX_PARENTS, crit) as tt, Learner(t, None, crit) as L:
                empty = L.score()
                got = L.optimal(tt, allowed=allowed)
                assert sorted((u, v) for v, ps in enumerate(L.parents()) for u in ps) == sorted(map(tuple, d[name]["edges"])), name
                assert L.score() == d[name]["score"] < empty and got["value"] == d[name]["value"] and len(d[name]["edges"]) > 0, name
        assert all(u < v for u, v in d["mdl_lower"]["edges"]) and d["mdl_lower"]["score"] >= d["mdl"]["score"] - OR.margin(13, abs(d["mdl"]["score"]))
    assert all(sum(1 for e in d[name]["edges"] if e[1] == v) <= MAX_PARENTS for name in ("mdl", "aic", "bdeu") for v in range(model.n))
