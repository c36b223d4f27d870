"""The hill-climbing restatement (tests/climb_refs.py) on libm's terms, without a GPU: every run keeps its graph a DAG within the
in-degree bound, never ends above where it started, a greedy run that stops at a local optimum has no improving move by a second,
literal routine, and the rows of RUNS reach the cases they were written for -- so the GPU test, which replays the same rows over
the device's terms, compares those cases too."""
import pytest

import climb_refs as CR
from bayesiannetwork_amd.learning import CLIMB_CAP, CLIMB_LOCAL_OPTIMUM, CLIMB_NO_MOVE, CLIMB_TRACE_DTYPE

_RESULTS = {}


def test_the_restatement_and_the_binding_name_the_same_flags_and_record():
    from bayesiannetwork_amd import _lib
    import ctypes
    assert (CR.END_NO_MOVE, CR.END_OPTIMUM, CR.END_CAP) == (CLIMB_NO_MOVE, CLIMB_LOCAL_OPTIMUM, CLIMB_CAP) == (1, 2, 4)
    assert CLIMB_TRACE_DTYPE.itemsize == 32 and ctypes.sizeof(_lib.ClimbParams) == 32
    assert any(name == "bn_learn_climb" for name, _, _ in _lib.SYMBOLS)
    assert CR.WAVES == 4   # kClimbWaves of bn_learn_climb.hpp


def results(name):
    """(Problem, arguments, the runs' records, the events of all of them); made once per row."""
    if name not in _RESULTS:
        pb, kw, runs = CR.run_setup(name)
        events = {}
        _RESULTS[name] = (pb, kw, [CR.climb_run(pb, j=j, events=events, **kw) for j in range(runs)], events)
    return _RESULTS[name]


@pytest.mark.parametrize("name", list(CR.RUNS))
def test_every_graph_of_a_run_is_a_dag_within_the_bound_and_the_best_is_no_worse_than_the_start(name):
    pb, kw, recs, _ = results(name)
    over = max(len(p) for p in pb.start)   # a start above the bound may stay there; nothing may grow past it
    for r in recs:
        assert len(r["trace"]) == r["steps"] == len(r["graphs"])
        for g in r["graphs"] + [r["parents"]]:
            assert CR.is_dag(g) and all(len(p) <= max(pb.mp, over) for p in g)
        assert r["score"] <= r["start_score"]
        assert r["best_step"] <= r["steps"] and r["improving"] <= r["steps"] and r["flags"] in (1, 2, 4)
        assert r["score"] == pb.score(r["ll"], r["params"])
        # the moves of the trace were legal where they were made, by the literal routine
        parents, ll = [list(p) for p in pb.start], None
        if r["perturbed"] == 0:
            ll = [pb.term(v, parents[v]) for v in range(pb.n)]
            for (kind, frm, to, d_bits, _), after in zip(r["trace"], r["graphs"]):
                legal = CR.literal_moves(pb, parents, ll)
                mid = (kind * pb.n + frm) * pb.n + to
                assert mid in legal and CR.bits(legal[mid]) == d_bits
                parents = after
                ll = [pb.term(v, parents[v]) for v in range(pb.n)]


@pytest.mark.parametrize("name", [name for name, row in CR.RUNS.items() if row[5] == 0])
def test_a_greedy_run_at_a_local_optimum_has_no_improving_move(name):
    pb, kw, recs, _ = results(name)
    ended = [r for r in recs if r["flags"] == CR.END_OPTIMUM]
    for r in ended:
        assert r["best_step"] == r["steps"] == r["improving"]          # every step improved: the last graph is the best
        assert r["final_parents"] == r["parents"]
        legal = CR.literal_moves(pb, r["final_parents"], r["final_ll"])
        assert legal == CR.moves_of(pb, r["final_parents"], r["final_ll"])
        assert not any(d < 0 for d in legal.values())
    assert ended or name == "n64_path_cap" or name == "n64_empty_greedy"


def test_the_rows_reach_what_they_are_there_for():
    ev = {name: results(name)[3] for name in CR.RUNS}
    recs = {name: results(name)[2] for name in CR.RUNS}
    assert ev["ties6_greedy"].get("tie_by_id", 0) > 0 and ev["ties6_tabu_bdeu"].get("tie_by_id", 0) > 0
    assert all(ev[name].get("refused_cycle", 0) > 0 for name in ("n6_greedy_aic", "n33_greedy_mdl", "n64_path_cap"))
    assert ev["n6_second_path"].get("refused_second_path", 0) > 0
    assert all(ev[name].get("refused_mp", 0) > 0 for name in ("n33_tabu_aic_mp2", "n33_dense_bdeu", "n64_dense_mp1"))
    assert ev["bigk_nan"].get("refused_nan", 0) > 0
    assert all(ev[name].get("tabu_changed_choice", 0) > 0 for name in ("n6_tabu_mdl", "n33_tabu_aic_mp2"))
    assert any(r["best_step"] < r["steps"] for r in recs["n6_tabu_mdl"])
    assert any(r["tabu_legal"] > 0 for r in recs["n6_tabu_mdl"])
    assert any(r["perturbed"] > 0 for r in recs["n6_tabu_mdl"][1:]) and recs["n6_tabu_mdl"][0]["perturbed"] == 0
    flags = {name: [r["flags"] for r in recs[name]] for name in CR.RUNS}
    assert flags["n2_no_move"] == [CR.END_NO_MOVE] and recs["n2_no_move"][0]["steps"] == 1
    assert flags["n6_greedy_aic"] == [CR.END_OPTIMUM] and flags["n33_greedy_mdl"] == [CR.END_OPTIMUM]
    assert flags["n33_reversed_mdl"] == [CR.END_OPTIMUM] and ev["n33_reversed_mdl"].get("reverse_applied", 0) >= 10
    assert flags["n64_path_cap"] == [CR.END_CAP] and recs["n64_path_cap"][0]["steps"] == 6
    for kind in CR.KINDS:   # every kind of move is applied somewhere
        assert any(e.get(kind + "_applied", 0) > 0 for e in ev.values()), kind


def test_the_choice_is_the_smallest_delta_then_the_lowest_id_and_zeros_tie():
    n = 4
    moves = {7: -1.0, 3: -2.0, 9: -2.0, 13: 0.5}     # from 1 to 3, 0 to 3, 2 to 1, 3 to 1
    assert CR.pick(moves, set(), n) == (3, -2.0, 0, 2)
    assert CR.pick(moves, {frozenset((0, 3))}, n) == (9, -2.0, 1, 1)        # id 3 is from 0 to 3
    assert CR.pick({5: 0.0, 2: -0.0}, set(), n)[0] == 2 and CR.pick({5: -0.0, 2: 0.0}, set(), n)[0] == 2
    assert CR.pick({}, set(), n)[0] is None
    assert CR.pick({6: 1.0}, {frozenset((1, 2))}, n) == (None, 0.0, 1, 0)   # id 6 is from 1 to 2
