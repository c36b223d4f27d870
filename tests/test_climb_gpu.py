"""Tabu hill climbing on the GPU (bn_learn_climb of include/bn_mi355x.h; bayesiannetwork_amd.learning.Learner.climb,
HillClimbing) against tests/climb_refs.py.

A run draws nothing but its perturbation and every delta is made of table entries by plain fp64 operations, so the restated run
replayed over the DEVICE's own fetched term rows must agree with the kernel in every bit: scores, counts, masks and the trace.
tests/test_climb_refs.py shows, on libm's terms, that the rows of climb_refs.RUNS reach ties, refusals, tabu exclusions and every
way of ending; the asserts on `events` below show the same over the device's terms for the rows where it matters."""
import ctypes

import numpy as np
import pytest

import anneal_refs as AR
import bd_refs as BD
import climb_refs as CR
import learning_refs as LR
from bayesiannetwork_amd import _lib

pytestmark = pytest.mark.gpu

COUNTS = ("steps", "improving", "perturbed", "best_step", "flags", "tabu_legal")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def info_table(table):
    from bayesiannetwork_amd.evaluation import InfoTable
    return InfoTable(table.pats, table.counts, table.k, device=0)


def device_criterion(criterion):
    return BD.BDEU1.criterion() if criterion == "bdeu" else criterion


def run_on_device(name, runs=None, trace_run=None, want_rows=True):
    """(device records, term rows, what the learner holds afterwards) of one row of climb_refs.RUNS."""
    from bayesiannetwork_amd.learning import Learner, TermTable, score_groups
    inp, q, criterion, mp, tabu_len, max_worse, max_steps, perturb, n_runs, seed, start = CR.RUNS[name]
    runs = n_runs if runs is None else runs
    crit = device_criterion(criterion)
    _, table = CR.climb_input(inp)
    with info_table(table) as t, TermTable(t, q, crit) as tt:
        rows = [tt.row(c) for c in range(table.n)] if want_rows else None
        with Learner(t, start, crit) as L:
            rec = L.climb(tt, tabu_len, max_worse, runs, perturb, seed, max_parents=mp, max_steps=max_steps, trace_run=trace_run)
            parents = L.parents()
            rescored = [x[0] for x in score_groups(t, [(v, parents[v], []) for v in range(table.n)], criterion=crit)]
            after = (L.score(), L.terms(), parents, rescored, L.info("climb_runs"), L.info("climb_steps"), L.info("climb_ns"))
    return rec, rows, after


def compare(rec, j, w):
    assert bits([rec["score"][j]])[0] == CR.bits(w["score"]), j
    assert tuple(int(rec[key][j]) for key in COUNTS) == tuple(w[key] for key in COUNTS), j
    assert [int(x) for x in rec["masks"][j]] == w["masks"], j


@pytest.mark.parametrize("name", list(CR.RUNS))
def test_runs_equal_the_restated_run_bit_for_bit(bnlib, name):
    n_runs = CR.RUNS[name][8]
    trace_run = n_runs - 1
    rec, rows, after = run_on_device(name, trace_run=trace_run)
    pb, kw, _ = CR.run_setup(name, rows)
    events = {}
    want = [CR.climb_run(pb, j=j, events=events, **kw) for j in range(n_runs)]
    for j, w in enumerate(want):
        compare(rec, j, w)
    got = [(int(x["kind"]), int(x["from"]), int(x["to"]), int(x["d_bits"]), int(x["current_bits"])) for x in rec["trace"]]
    assert got == want[trace_run]["trace"] and len(got) == want[trace_run]["steps"]
    # what the row is there for, over the DEVICE's terms
    needs = {"ties6_greedy": ["tie_by_id"], "ties6_tabu_bdeu": ["tie_by_id"], "n6_second_path": ["refused_second_path"],
             "bigk_nan": ["refused_nan"], "n33_tabu_aic_mp2": ["refused_mp", "tabu_changed_choice"], "n33_dense_bdeu": ["refused_mp"],
             "n6_tabu_mdl": ["tabu_changed_choice", "delete_applied"], "n33_reversed_mdl": ["reverse_applied"],
             "n64_path_cap": ["refused_cycle"], "n64_dense_mp1": ["refused_mp"]}
    assert all(events.get(key, 0) > 0 for key in needs.get(name, [])), events
    ends = {"n2_no_move": CR.END_NO_MOVE, "n6_greedy_aic": CR.END_OPTIMUM, "n33_greedy_mdl": CR.END_OPTIMUM, "n64_path_cap": CR.END_CAP}
    assert name not in ends or [w["flags"] for w in want] == [ends[name]]
    assert name != "n6_tabu_mdl" or any(w["best_step"] < w["steps"] for w in want)
    # the winner: the strictly smallest score, the lowest run among equals; the learner holds its graph and terms
    scores = [w["score"] for w in want]
    winner = scores.index(min(scores))
    assert rec["winner"] == winner
    score, (ll, params), parents, rescored, climb_runs, climb_steps, ns = after
    assert bits([score])[0] == CR.bits(want[winner]["score"]) and score == pb.score(ll, params)
    assert np.array_equal(bits(ll), bits(want[winner]["ll"])) and params == want[winner]["params"]
    assert parents == want[winner]["parents"]
    assert np.array_equal(bits(rescored), bits(ll))                   # the graph rescored through score_groups: the same terms
    assert climb_runs == n_runs and climb_steps == sum(w["steps"] for w in want) and ns > 0


def test_a_run_does_not_depend_on_the_number_of_runs_or_its_place_in_a_workgroup(bnlib):
    name, many = "n33_tabu_aic_mp2", 4 * CR.WAVES + 1     # four full workgroups and a fifth with one wave
    full, rows, _ = run_on_device(name, runs=many)
    for j in (0, 2, 5):
        part = run_on_device(name, runs=j + 1, want_rows=False)[0]
        for key in COUNTS + ("score", "masks"):
            assert np.array_equal(np.atleast_1d(part[key][j]).view(np.uint8), np.atleast_1d(full[key][j]).view(np.uint8)), (j, key)
    pb, kw, _ = CR.run_setup(name, rows)
    for j in (CR.WAVES - 1, CR.WAVES, many - 1):          # the last wave of a workgroup, the first of the next, the lone last one
        compare(full, j, CR.climb_run(pb, j=j, **kw))
    assert len({int(x) for x in bits(full["score"])}) > 1   # the perturbed starts do lead to different graphs


def test_among_equal_scores_the_lowest_run_wins(bnlib):
    """Without perturbation every run is run 0: equal scores in every bit, and the winner is run 0, not the last."""
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = AR.anneal_input("n6")
    with info_table(table) as t, TermTable(t, 3) as tt, Learner(t, None, "aic") as L:
        rec = L.climb(tt, runs=6)
        assert len({int(x) for x in bits(rec["score"])}) == 1 and rec["winner"] == 0
        assert bits([L.score()])[0] == bits(rec["score"])[0]
        assert [sum(1 << u for u in p) for p in L.parents()] == [int(x) for x in rec["masks"][0]]


def test_argument_errors_launch_nothing(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = AR.anneal_input("n5")
    lib = _lib.lib()
    with info_table(table) as t, info_table(table) as other, TermTable(t, 2) as tt, TermTable(other, 2) as tt_other, \
            TermTable(t, 2, BD.BDEU1.criterion()) as tt_bdeu:
        with Learner(t, None, "aic") as L:
            for bad in (dict(runs=0), dict(runs=(1 << 16) + 1), dict(tabu_len=-1), dict(tabu_len=65), dict(max_steps=(1 << 20) + 1),
                        dict(perturb=(1 << 16) + 1), dict(max_parents=0), dict(runs=4, trace_run=4), dict(runs=4, trace_run=-2)):
                with pytest.raises(_lib.BnError) as ei:
                    L.climb(tt, **bad)
                assert ei.value.code == _lib.BN_ERR_ARG, bad
            with pytest.raises(_lib.BnError) as ei:
                L.climb(tt_other)
            assert ei.value.code == _lib.BN_ERR_ARG and "another table" in str(ei.value)
            with pytest.raises(ValueError):
                L.climb(tt_bdeu)
            p = _lib.ClimbParams(2, 0, 0, 0, 0, -1, 0, 0)       # the same refusal from the library itself
            w = ctypes.c_int32()
            assert lib.bn_learn_climb(L._h, tt_bdeu._h, ctypes.byref(p), 1, 0, None, None, None, None, ctypes.byref(w)) == _lib.BN_ERR_ARG
            assert b"term table" in lib.bn_last_error()
            assert L.info("climb_runs") == 0 and L.info("climb_steps") == 0 and L.info("edges") == 0
            rec = L.climb(tt, max_parents=5, max_steps=50)                                                   # (above q: the table's bound holds)
            assert L.info("climb_runs") == 1 and all(bin(int(m)).count("1") <= 2 for m in rec["masks"][0])
        with Learner(t, [[], [], [], [], [0, 1, 2]], "aic") as L:      # a starting family over q = 2
            with pytest.raises(_lib.BnError) as ei:
                L.climb(tt)
            assert ei.value.code == _lib.BN_ERR_ARG and "3 parents" in str(ei.value) and L.info("climb_runs") == 0
        pats = np.zeros((3, 65), np.uint8)
        pats[1, :] = 1
        with InfoTable(pats, np.ones(3, np.uint64), [2] * 65, device=0) as t65, Learner(t65, None, "aic") as L65:
            with pytest.raises(_lib.BnError) as ei:
                L65.climb(tt)
            assert ei.value.code == _lib.BN_ERR_ARG and "65" in str(ei.value) and "64" in str(ei.value) and L65.info("climb_runs") == 0


def test_hill_climbing_end_to_end(bnlib):
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import MDL
    from bayesiannetwork_amd.learning import HillClimbing, Learner, structure_model
    model, table, _, _, _ = LR.learning_input("alarm2k_mdl")
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table) as t:
        hc = HillClimbing("mdl", t, max_parents=3, runs=8, seed=5)
        learned, score = hc(start, tabu_len=10, max_worse=10, perturb=20, max_steps=200)
        learned.validate()                                            # a DAG with CPTs of the right shape
        parents = [learned.parents(v).tolist() for v in range(model.n)]
        assert all(len(p) <= 3 for p in parents) and sum(map(len, parents)) > 0
        with Learner(t, None, "mdl") as L0, Learner(t, learned, "mdl") as L1:
            assert score < L0.score() and bits([L1.score()])[0] == bits([score])[0]   # the public API gives the score back, bit for bit
        with Engine(learned, device=0) as eng:
            assert abs(MDL(t)(eng) - score) <= LR.graph_bound(table, parents, "mdl")
        first = dict(hc.last)
        assert first["term_entries"] == 37 * 7807 and first["climb_runs"] == 8 and first["climb_steps"] > 8 and 0 <= first["winner"] < 8
        greedy_model, greedy_score = hc(start)                        # the classic climb: the same term table, no second build
        assert hc.last["term_passes"] == first["term_passes"] and greedy_score < L0_score(t)
        assert all(int(f) in (CR.END_OPTIMUM, CR.END_CAP) for f in hc.records["flags"]) and hc.records["winner"] == 0
        hc.close()


def L0_score(t):
    from bayesiannetwork_amd.learning import Learner
    with Learner(t, None, "mdl") as L0:
        return L0.score()
