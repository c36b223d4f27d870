"""The host halves of constraint-based learning as stand-alone programs: tests/cpp/test_ci_plan.cpp (ranks, groups, chunks, stopping
and refusals of bn_ci_plan.cpp, property by property) and tests/cpp/test_ci_orient.cpp (bn_ci_orient.cpp against tests/pc_refs.py on
the same random graphs), each compiled with its source under AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of
its own; and, on the GPU, bn::learning::pc of the C++ drop-in (tests/cpp/test_pc_algorithm.cpp) against the Python learner."""
import json
import os
import subprocess

import numpy as np
import pytest

import pc_refs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(tmp_path, name, source):
    exe = str(tmp_path / name)
    cmd = SAN + ["-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                 os.path.join(CSRC, source), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_ci_planner_properties(tmp_path):
    out = subprocess.run([build(tmp_path, "test_ci_plan", "bn_ci_plan.cpp")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
    print(out.stdout.strip())


def random_case(rng):
    """A random skeleton with a separating set (or none) for every non-adjacent pair: not necessarily one PC could produce, which is
    the point -- conflicts between v-structures and PDAGs without an extension occur."""
    n = int(rng.integers(2, 8))
    skel = np.triu((rng.random((n, n)) < rng.uniform(0.2, 0.8)).astype(np.uint8), 1)
    skel = skel + skel.T
    sepsets = {}
    for x in range(n):
        for y in range(x + 1, n):
            if not skel[x, y] and rng.random() < 0.85:
                others = [v for v in range(n) if v not in (x, y)]
                size = int(rng.integers(0, min(3, len(others)) + 1))
                sepsets[(x, y)] = tuple(sorted(int(v) for v in rng.choice(others, size=size, replace=False))) if size else ()
    return n, skel, sepsets


def test_orientation_equals_the_python_restatement(tmp_path):
    rng = np.random.default_rng(11)
    cases = [random_case(rng) for _ in range(300)]
    for name in ("collider", "chain", "collider_tail", "diamond"):   # and the results of the four small networks
        r = P.libm_result(name)
        cases.append((r["skeleton"].shape[0], r["skeleton"], r["sepsets"]))
    lines = [str(len(cases))]
    for n, skel, sepsets in cases:
        lines.append(f"{n} 3")
        lines.append(" ".join(str(int(v)) for v in skel.reshape(-1)))
        for x in range(n):
            for y in range(x + 1, n):
                s = sepsets.get((x, y))
                lines.append("-1" if s is None else " ".join(str(v) for v in (len(s),) + tuple(s)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([build(tmp_path, "test_ci_orient", "bn_ci_orient.cpp"), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    got = out.stdout.split("\n")

    def dag_text(par):
        return "none" if par is None else ";".join(f"{v}:" + "".join(f" {u}" for u in ps) for v, ps in enumerate(par))
    oriented = none = 0
    for i, (n, skel, sepsets) in enumerate(cases):
        cpdag = P.meek(P.orient_colliders(skel, sepsets))
        assert got[3 * i] == "".join(str(int(v)) for v in cpdag.reshape(-1)), (i, skel, sepsets)
        assert got[3 * i + 1] == dag_text(P.pdag_to_dag(cpdag)), (i, cpdag)
        assert got[3 * i + 2] == dag_text(P.pdag_to_dag(skel)), (i, skel)
        oriented += int((cpdag != cpdag.T).any())
        none += got[3 * i + 1] == "none"
    assert oriented > 50 and none > 5 and none < len(cases) - 50   # the cases exercise both outcomes


@pytest.mark.gpu
def test_cpp_pc_algorithm_equals_the_python_learner(bnlib, tmp_path):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import PC, cpdag_to_dag
    import learning_refs as LR
    model, table, _, _, _ = LR.learning_input("alarm2k_mdl")
    path = tmp_path / "samples.txt"
    path.write_text("".join(f"{int(c)} " + " ".join(str(int(s)) for s in row) + "\n" for row, c in zip(table.pats, table.counts)))
    exe = str(tmp_path / "test_pc_algorithm")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           os.path.join(ROOT, "tests", "cpp", "test_pc_algorithm.cpp"), "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}",
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"), str(path), "0.05", "2"], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        r = PC(0.05, 2)(t)
        parents = cpdag_to_dag(r.cpdag)
    assert d["n"] == model.n and d["alpha_refused"] is True
    assert np.array_equal(np.array(d["cpdag"], dtype=np.uint8).reshape(model.n, model.n), r.cpdag)
    assert sorted(map(tuple, d["edges"])) == sorted((u, v) for v, ps in enumerate(parents) for u in ps)
    for (a, b), s in r.sepsets.items():
        assert tuple(d["sepsets"][f"{a},{b}"]) == s
    assert len(d["sepsets"]) == len(r.sepsets)
