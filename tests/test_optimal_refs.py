"""The restated exact search (tests/optimal_refs.py, the contract of bn_learn_optimal in include/bn_mi355x.h) on a CPU, over libm's
terms (anneal_refs.libm_term, bd_refs for BDeu):

  * against an enumeration of every DAG (29 281 over five nodes, 543 over four) whose costs are added as Fractions: the restated
    DP's graph is a DAG within the bounds and its exact cost is within the derived margin 2 n 2^-52 max|R| of the true minimum;
  * ties: equal costs go to the smaller rank in step 1 and to the lowest sink in step 2, and the input reaches both;
  * the butterflies in any order of the bits give the same bytes;
  * the planner (bayesiannetwork_amd/csrc/bn_learn_optimal_plan.cpp) as a stand-alone program under the host sanitizers."""
import itertools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import anneal_refs as AR
import climb_refs as CR
import optimal_refs as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")

CASES = [("n5", c, mp) for c in ("aic", "mdl", "bdeu") for mp in (2, 4)] + [("bigk", "aic", 3)]


def problem(name, criterion, mp, allowed=None):
    _, table = OR.optimal_input(name)
    q = min(mp, table.n - 1)
    return OR.Problem(table.k, q, criterion, table.total, OR.cpu_rows(name, q, criterion), allowed)


def check_against_enumeration(pb, allowed=None):
    got = OR.optimal(pb)
    parents = got["parents"]
    assert CR.is_dag(parents) and all(len(p) <= pb.mp for p in parents)
    assert all(not math.isnan(pb.term(v, p)) for v, p in enumerate(parents))              # no family that is not eligible
    pos = {s: i for i, s in enumerate(got["order"])}
    assert sorted(got["order"]) == list(range(pb.n)) and all(pos[u] < pos[v] for v, p in enumerate(parents) for u in p)
    if allowed is not None:
        assert all(OR.mask_of(p) & ~allowed[v] == 0 for v, p in enumerate(parents))
    cost = OR.exact_cost(pb, parents)
    best, best_graph, count = OR.exact_min_by_enumeration(pb)
    assert cost is not None and best is not None and cost >= best
    assert cost - best <= Fraction(OR.margin(pb.n, got["max_abs_R"])), (float(cost), float(best), best_graph)
    assert abs(Fraction(got["value"]) - cost) <= Fraction(OR.margin(pb.n, got["max_abs_R"]))
    assert OR.bits_equal(got["value"], OR.replay_value(pb, got["order"], parents))
    return got, count


@pytest.mark.parametrize("name,criterion,mp", CASES)
def test_restated_dp_finds_the_enumerated_minimum(name, criterion, mp):
    pb = problem(name, criterion, mp)
    got, count = check_against_enumeration(pb)
    if name == "n5" and mp == 4:
        assert count == 29281 and len(OR.all_dags(5)) == 29281
    if name == "bigk":
        # the input is there for its NaN terms: some families within mp are not eligible, and the DP's costs hold +inf for them
        assert len(OR.all_dags(4)) == 543 and count < 543
        assert math.isnan(pb.term(3, [0, 1, 2])) and math.isinf(pb.family_cost(3, [0, 1, 2]))


@pytest.mark.parametrize("criterion", ["aic", "bdeu"])
def test_allowed_restricts_the_search_to_the_skeleton(criterion):
    model, _ = OR.optimal_input("n5")
    allowed = OR.skeleton_masks(model)
    assert 0 < sum(bin(a).count("1") for a in allowed) < 5 * 4
    free, _ = check_against_enumeration(problem("n5", criterion, 4))
    bound, count = check_against_enumeration(problem("n5", criterion, 4, allowed), allowed)
    assert count < 29281
    assert OR.exact_cost(problem("n5", criterion, 4), bound["parents"]) >= OR.exact_cost(problem("n5", criterion, 4), free["parents"])


def literal_best_parent_sets(pb):
    """Step 1 as its definition: per child and candidate set, the smallest (cost, rank) over every subset, as Python tuples."""
    n, m = pb.n, pb.n - 1
    costs, ranks = np.zeros((n, 1 << m)), np.zeros((n, 1 << m), dtype=np.uint32)
    for v in range(n):
        first_c, first_r = OR.first_cells(pb, v)
        for c in range(1 << m):
            sub, best = c, None
            while True:
                pair = (float(first_c[sub]), int(first_r[sub]))
                best = pair if best is None or pair < best else best
                if sub == 0:
                    break
                sub = (sub - 1) & c
            costs[v][c], ranks[v][c] = best
    return costs, ranks


def literal_best_sinks(pb, costs):
    n = pb.n
    R, sink = [0.0] * (1 << n), [0] * (1 << n)
    for W in sorted(range(1, 1 << n), key=lambda w: bin(w).count("1")):
        best = None
        for v in OR.nodes_of(W):
            val = R[W ^ (1 << v)] + float(costs[v][OR.squeeze(W ^ (1 << v), v)])
            if best is None or val < best:
                best, sink[W] = val, v
        R[W] = best
    return np.array(R), np.array(sink, dtype=np.uint8)


@pytest.mark.parametrize("name,criterion", [("ties6", "aic"), ("ties6", "bdeu"), ("n6", "mdl")])
def test_ties_go_to_the_smaller_rank_and_the_lowest_sink(name, criterion):
    pb = problem(name, criterion, 3)
    events = {}
    got = OR.optimal(pb, events, keep=True)
    lit_c, lit_r = literal_best_parent_sets(pb)
    assert got["costs"].tobytes() == lit_c.tobytes() and got["ranks"].tobytes() == lit_r.tobytes()
    lit_R, lit_sink = literal_best_sinks(pb, lit_c)
    assert got["R"].tobytes() == lit_R.tobytes() and got["sink"].tobytes() == lit_sink.tobytes()
    if name == "ties6":
        assert events.get("rank_tie", 0) > 0 and events.get("sink_tie", 0) > 0, events       # the input reaches both kinds of tie
        # ... and a tie decides a cell: somewhere the winner is the smaller of two ranks whose sets have the same cost
        v, c = 2, OR.squeeze(OR.mask_of([0, 4]), 2)
        assert pb.family_cost(2, [0]) == pb.family_cost(2, [4]) and AR.rank(6, 2, [0]) < AR.rank(6, 2, [4])
        assert got["ranks"][v][c] != AR.rank(6, 2, [4])


def test_the_order_of_the_bit_passes_does_not_matter():
    for name, criterion in (("ties6", "aic"), ("n6", "mdl"), ("bigk", "aic")):
        pb = problem(name, criterion, 3)
        base_c, base_r = OR.best_parent_sets(pb)
        m = pb.n - 1
        rng = np.random.default_rng(7)
        for order in [list(range(m))[::-1]] + [rng.permutation(m).tolist() for _ in range(3)]:
            c, r = OR.best_parent_sets(pb, bit_order=order)
            assert c.tobytes() == base_c.tobytes() and r.tobytes() == base_r.tobytes(), (name, order)


def test_squeeze_and_rank_relabel_alike():
    for n, v in itertools.product((2, 5, 13), (0, 1, 4)):
        if v >= n:
            continue
        for C in range(1 << min(n, 8)):
            if (C >> v) & 1:
                continue
            c = OR.squeeze(C, v)
            assert OR.unsqueeze(c, v) == C and OR.nodes_of(c) == [s - (s > v) for s in OR.nodes_of(C)]


def test_planner_stand_alone(tmp_path):
    exe = str(tmp_path / "test_optimal_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_optimal_plan.cpp"),
           os.path.join(CSRC, "bn_learn_optimal_plan.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.startswith("ok: "), out.stdout
