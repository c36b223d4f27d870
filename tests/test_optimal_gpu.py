"""The exact search on the GPU (bn_learn_optimal of include/bn_mi355x.h; bayesiannetwork_amd.learning.Learner.optimal,
OptimalSearch) against tests/optimal_refs.py.

Every cost is made of table entries by plain fp64 operations, min does not round and ties have a stated winner, so the restated
search over the DEVICE's own fetched term rows must agree with the kernels in every bit: value, order, masks, and what the learner
holds afterwards.  The sizes are the edges of the tiling: a partial tile (n <= 12), exactly one tile (13), one and three bits above
it (14, 16), seven (20, one strided pass) and nine (22, two strided passes), and n = 1, 2.  tests/test_optimal_refs.py shows on a CPU
that the restatement finds the enumerated minimum."""
import ctypes
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import bd_refs as BD
import climb_refs as CR
import learning_refs as LR
import optimal_refs as OR
from bayesiannetwork_amd import _lib

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def info_table(table):
    from bayesiannetwork_amd.evaluation import InfoTable
    return InfoTable(table.pats, table.counts, table.k, device=0)


def device_criterion(criterion):
    return {"bdeu": BD.BDEU1.criterion, "k2": BD.K2S.criterion}[criterion]() if criterion in ("bdeu", "k2") else criterion


def learner_score(pb, ll, params):
    return LR.score_arith(ll, params, pb.criterion, pb.total) if pb.penalised else BD.likelihood_alone(ll)


def run_on_device(name, q, criterion, mp=None, allowed=None, twice=False):
    """(the device's result, the restatement's over the device's term rows, what the learner holds afterwards, the problem)."""
    from bayesiannetwork_amd.learning import Learner, TermTable, _allowed_masks, score_groups
    crit = device_criterion(criterion)
    _, table = OR.optimal_input(name)
    with info_table(table) as t, TermTable(t, q, crit) as tt:
        rows = [tt.row(c) for c in range(table.n)]
        with Learner(t, None, crit) as L:
            got = L.optimal(tt, max_parents=mp, allowed=allowed)
            parents = L.parents()
            rescored = [x[0] for x in score_groups(t, [(v, parents[v], []) for v in range(table.n)], criterion=crit)]
            after = {"score": L.score(), "terms": L.terms(), "parents": parents, "rescored": rescored, "ns": L.info("optimal_ns"),
                     "cells": L.info("optimal_cells"), "bytes": L.info("optimal_bytes")}
            if twice:
                after["again"] = L.optimal(tt, max_parents=mp, allowed=allowed)
                after["ns_again"] = L.info("optimal_ns")
    words = None if allowed is None else [int(x) for x in _allowed_masks(allowed, table.n)]
    pb = OR.Problem(table.k, min(q if mp is None else mp, q), criterion, table.total, rows, words)
    return got, after, pb


def compare(got, after, pb, want):
    n = pb.n
    assert bits([got["value"]])[0] == CR.bits(want["value"])
    assert got["order"].tolist() == want["order"] and [int(x) for x in got["masks"]] == want["masks"]
    assert got["parents"] == want["parents"] and after["parents"] == want["parents"]
    ll, params = after["terms"]
    assert np.array_equal(bits(ll), bits(want["ll"])) and params == want["params"]
    assert bits([after["score"]])[0] == CR.bits(learner_score(pb, want["ll"], want["params"]))
    assert np.array_equal(bits(after["rescored"]), bits(ll))          # the graph rescored through score_groups: the same term bits
    assert after["cells"] == n << (n - 1) and after["bytes"] == 12 * (n << (n - 1)) + 9 * (1 << n) and after["ns"] > 0
    # the result is a graph the bounds admit, and adding its costs up along the order gives the value again
    assert CR.is_dag(got["parents"]) and all(len(p) <= pb.mp and math.isfinite(pb.family_cost(v, p)) for v, p in enumerate(got["parents"]))
    assert OR.bits_equal(got["value"], OR.replay_value(pb, want["order"], want["parents"]))


# (input, the table's q, criterion, max_parents handed to the call)
FULL = [("n1", 1, "aic", None), ("n2", 1, "mdl", None), ("n5", 3, "aic", None), ("n5", 3, "bdeu", None), ("n6", 3, "mdl", None),
        ("n6", 3, "k2", None), ("ties6", 3, "aic", None), ("ties6", 3, "bdeu", None), ("bigk", 3, "aic", None), ("bigk", 3, "mdl", None),
        ("o13", 3, "aic", None), ("o13", 3, "mdl", None), ("o14", 2, "aic", None), ("o14", 2, "bdeu", None),
        ("o16", 3, "aic", None), ("o16", 3, "mdl", None), ("o16", 3, "bdeu", None), ("o16", 3, "k2", None), ("o16", 3, "aic", 2)]


@pytest.mark.parametrize("name,q,criterion,mp", FULL)
def test_equals_the_restated_search_bit_for_bit(bnlib, name, q, criterion, mp):
    got, after, pb = run_on_device(name, q, criterion, mp)
    events = {}
    want = OR.optimal(pb, events)
    compare(got, after, pb, want)
    if name == "ties6":
        assert events.get("rank_tie", 0) > 0 and events.get("sink_tie", 0) > 0, events   # both kinds of tie, over the device's terms
    if name == "bigk":
        assert any(math.isnan(x) for row in pb.rows for x in row)
    if mp is not None:
        assert pb.mp == mp < q and max(len(p) for p in got["parents"]) <= mp


def test_allowed_as_the_models_skeleton(bnlib):
    model, _ = OR.optimal_input("o13")
    allowed = OR.skeleton_masks(model)
    got, after, pb = run_on_device("o13", 3, "aic", allowed=allowed)
    compare(got, after, pb, OR.optimal(pb))
    assert all(OR.mask_of(p) & ~allowed[v] == 0 for v, p in enumerate(got["parents"])) and sum(map(len, got["parents"])) > 0
    free, _, free_pb = run_on_device("o13", 3, "aic")
    assert free["value"] <= got["value"]                               # fewer graphs: min over a subset, term by term the same adds
    lists = [OR.nodes_of(a) for a in allowed]                          # the same restriction as per-node lists
    assert run_on_device("o13", 3, "aic", allowed=lists)[0]["masks"].tobytes() == got["masks"].tobytes()


def test_allowed_from_a_pc_result(bnlib):
    from bayesiannetwork_amd.learning import PC
    _, table = OR.optimal_input("o13")
    with info_table(table) as t:
        pc = PC(alpha=0.05, max_cond=2)(t)
    skeleton = [OR.mask_of(np.nonzero(pc.skeleton[v])[0]) for v in range(table.n)]
    assert 0 < sum(bin(a).count("1") for a in skeleton) < 13 * 12
    got, after, pb = run_on_device("o13", 3, "mdl", allowed=pc)
    assert pb.allowed == skeleton
    compare(got, after, pb, OR.optimal(pb))
    assert all(OR.mask_of(p) & ~skeleton[v] == 0 for v, p in enumerate(got["parents"]))


@pytest.mark.parametrize("name,criterion", [("o16", "mdl"), ("n6", "aic")])
def test_the_optimum_bounds_the_heuristics(bnlib, name, criterion):
    """The Fraction-exact cost of the graphs the climb (64 runs, tabu 8) and the annealing (64 chains) end with is no smaller than
    the exact search's, less the derived margin 2 n 2^-52 max|R| (optimal_refs.margin)."""
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = OR.optimal_input(name)
    with info_table(table) as t, TermTable(t, 3, criterion) as tt:
        rows = [tt.row(c) for c in range(table.n)]
        pb = OR.Problem(table.k, 3, criterion, table.total, rows)
        with Learner(t, None, criterion) as L:
            best = L.optimal(tt)
        want = OR.optimal(pb)
        assert best["parents"] == want["parents"]
        floor = OR.exact_cost(pb, best["parents"]) - Fraction(OR.margin(pb.n, want["max_abs_R"]))
        with Learner(t, None, criterion) as L:
            L.climb(tt, tabu_len=8, max_worse=8, runs=64, perturb=6, seed=3, max_steps=400)
            climbed = L.parents()
        with Learner(t, None, criterion) as L:
            L.anneal(tt, 8.0, 0.05, 0.97, chains=64, seed=4, rule="metropolis", max_proposals=4000)
            annealed = L.parents()
    for found in (climbed, annealed):
        assert CR.is_dag(found) and all(len(p) <= 3 for p in found)
        assert OR.exact_cost(pb, found) >= floor, found


@pytest.mark.parametrize("name", ["o20", "o22"])
def test_replay_beyond_the_host_restatement(bnlib, name):
    """20 and 22 nodes (q = 2): no host DP at this size.  The result is checked by its properties and by adding the costs up again
    in the DP's order.  The climb's score is the learner's arithmetic on its own graph, another order of additions than R[V]'s: the
    comparison carries the margin of optimal_refs.margin with max|R| = R[V] (under AIC every cost is positive, so R grows with W)."""
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = OR.optimal_input(name)
    n = table.n
    with info_table(table) as t, TermTable(t, 2, "aic") as tt:
        rows = [tt.row(c) for c in range(n)]
        with Learner(t, None, "aic") as L:
            got = L.optimal(tt)
            assert L.parents() == got["parents"] and L.info("optimal_cells") == n << (n - 1)
            score = L.score()
        with Learner(t, None, "aic") as L:
            L.climb(tt, tabu_len=8, max_worse=8, runs=16, perturb=6, seed=5, max_steps=400)
            climb_score = L.score()
    pb = OR.Problem(table.k, 2, "aic", table.total, rows)
    order, parents = got["order"].tolist(), got["parents"]
    assert sorted(order) == list(range(n))
    pos = {s: i for i, s in enumerate(order)}
    assert all(pos[u] < pos[v] for v, p in enumerate(parents) for u in p)
    assert all(len(p) <= 2 and math.isfinite(pb.family_cost(v, p)) for v, p in enumerate(parents)) and sum(map(len, parents)) > 0
    assert OR.bits_equal(got["value"], OR.replay_value(pb, order, parents))
    slack = OR.margin(n, abs(got["value"]))
    assert all(pb.family_cost(v, p) > 0 for v, p in enumerate(parents)) and got["value"] <= climb_score + slack
    assert abs(score - got["value"]) <= slack
    # a sink's parents are its best set among the nodes before it: no other eligible subset of them costs less
    for i, s in enumerate(order):
        before = order[:i]
        costs = [pb.family_cost(s, list(S)) for j in range(3) for S in itertools.combinations(before, j)]
        assert pb.family_cost(s, parents[s]) == min(costs)


def test_argument_errors_launch_nothing(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = OR.optimal_input("n5")
    lib = _lib.lib()
    start = [[], [0], [], [2], []]
    with info_table(table) as t, info_table(table) as other, TermTable(t, 2) as tt, TermTable(other, 2) as tt_other, \
            TermTable(t, 2, BD.BDEU1.criterion()) as tt_bdeu, Learner(t, start, "aic") as L:
        def refused(text, **kw):
            with pytest.raises(_lib.BnError) as ei:
                L.optimal(kw.pop("table", tt), **kw)
            assert ei.value.code == _lib.BN_ERR_ARG and text in str(ei.value), str(ei.value)
            assert L.parents() == start and L.info("optimal_ns") == 0 and L.info("optimal_cells") == 0
        refused("max_parents 0", max_parents=0)
        refused("allowed[4]", allowed=[0, 0, 0, 0, 1 << 5])
        refused("another table", table=tt_other)
        with pytest.raises(ValueError):
            L.optimal(tt_bdeu)
        p = _lib.OptimalParams(2, 0, None, 0)                          # the same refusal from the library itself
        value = ctypes.c_double()
        assert lib.bn_learn_optimal(L._h, tt_bdeu._h, ctypes.byref(p), ctypes.byref(value), None, None) == _lib.BN_ERR_ARG
        assert b"term table" in lib.bn_last_error() and L.parents() == start and L.info("optimal_ns") == 0
        assert lib.bn_learn_optimal(L._h, tt._h, None, ctypes.byref(value), None, None) == _lib.BN_ERR_ARG
        got = L.optimal(tt, max_parents=7)                             # above q: the table's bound holds
        assert max(len(p) for p in got["parents"]) <= 2 and L.info("optimal_ns") > 0 and L.parents() == got["parents"]
    pats = np.zeros((3, 25), np.uint8)
    pats[1, :] = 1
    with InfoTable(pats, np.ones(3, np.uint64), [2] * 25, device=0) as t25, TermTable(t25, 1) as tt25, Learner(t25, None, "aic") as L25:
        with pytest.raises(_lib.BnError) as ei:
            L25.optimal(tt25)
        assert ei.value.code == _lib.BN_ERR_ARG and "25 nodes" in str(ei.value) and "24" in str(ei.value)
        assert L25.info("optimal_ns") == 0 and L25.info("edges") == 0


def test_a_second_call_gives_the_same_bytes(bnlib):
    got, after, _ = run_on_device("o14", 2, "mdl", twice=True)
    again = after["again"]
    assert bits([got["value"]])[0] == bits([again["value"]])[0] and got["order"].tobytes() == again["order"].tobytes()
    assert got["masks"].tobytes() == again["masks"].tobytes() and after["ns_again"] > after["ns"]


def test_optimal_search_end_to_end(bnlib):
    from bayesiannetwork_amd.learning import HillClimbing, Learner, OptimalSearch, structure_model
    model, table = OR.optimal_input("o13")
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table) as t:
        opt = OptimalSearch("mdl", t, max_parents=3)
        learned, score = opt(start)
        learned.validate()
        parents = [learned.parents(v).tolist() for v in range(model.n)]
        assert parents == opt.records["parents"] and all(len(p) <= 3 for p in parents)
        with Learner(t, learned, "mdl") as L1:
            assert bits([L1.score()])[0] == bits([score])[0]
        assert opt.last["optimal_cells"] == 13 << 12 and opt.last["optimal_ns"] > 0
        hc = HillClimbing("mdl", t, max_parents=3, runs=8, seed=5)
        _, climbed = hc(start, tabu_len=8, max_worse=8, perturb=6, max_steps=200)
        assert score <= climbed + OR.margin(13, abs(score))
        restricted, bound_score = opt(start, allowed=OR.skeleton_masks(model))
        assert bound_score >= score - OR.margin(13, abs(score))
        hc.close()
        opt.close()
