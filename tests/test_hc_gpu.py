"""Hierarchical clustering with stochastic pruning on the GPU (bn_learn_hc of include/bn_mi355x.h; bayesiannetwork_amd.learning
Learner.hc, StepwiseStructureHC) against tests/hc_refs.py.

Runs are compared bit for bit with the restated run (which tests/test_hc_refs.py holds equal to the literal transcription of the
reference's loop) replayed over the DEVICE's own fetched terms and the device's own similarity matrix (InfoTable.pair_entropies):
every arithmetic step but pow is then the same on both sides, and before any comparison the replay shows that no pruning decision
has |u - p| <= 2^-40 * max(u, p) -- none is left out.  A failure of that margin says: change the seed.

Two of the cases differ from their one-line statement, for reasons tests/hc_refs.py spells out: alpha = 1 ends after ONE merge
only where three nodes are all there is (t3_alpha1; on n5 the untouched clusters go on merging: n // 2 merges), and bigk's own 500
samples never keep an edge between 255-state nodes, so the NaN refusal is shown on bigk_counts (the same arities, weighted
patterns) while bigk itself is still compared bit for bit; n6 with q = 2 refuses at in-degree 1 over the q = 2 table (no node of
n6 earns a second parent) and n33 shows the refusal at in-degree 3.

The rows of hc_refs.NEW_ROWS put lists of 528 and 2 016 entries with equal maxima through the pick (several strided entries per
lane, ties across lanes) and a caller's NaN, +inf and -inf through the keys, the compaction and pow; for each the replay over the
device's terms must still reach the forms the row exists for."""
import math

import numpy as np
import pytest

import anneal_refs as AR
import hc_refs as HR
import learning_refs as LR
from bayesiannetwork_amd import _lib

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def info_table(table):
    from bayesiannetwork_amd.evaluation import InfoTable
    return InfoTable(table.pats, table.counts, table.k, device=0)


def device_term(rows, n):
    """term(child, parents) over the fetched rows of a TermTable."""
    return lambda child, parents: float(rows[child][AR.rank(n, child, parents)])


def run_on_device(name, runs=None, trace_run=None):
    """(device records, Problem over the device's terms, S as the device read it, alpha, runs, seed, the learner afterwards)."""
    from bayesiannetwork_amd.learning import Learner, TermTable
    inp, q, criterion, alpha, n_runs, seed, kind = HR.RUNS[name]
    runs = n_runs if runs is None else runs
    _, table = HR.hc_input(inp)
    with info_table(table) as t, TermTable(t, q) as tt:
        rows = [tt.row(c) for c in range(table.n)]
        mi = t.pair_entropies()["mi"] if kind == "mi" else None
        with Learner(t, None, criterion) as L:
            rec = L.hc(tt, alpha, runs, seed, max_parents=HR.MAX_PARENTS.get(name), trace_run=trace_run,
                       similarity=None if kind == "mi" else HR.similarity_matrix(kind, table.n))
            after = (L.score(), L.terms(), L.parents(), L.info("hc_runs"), L.info("hc_merges"), L.info("hc_ns"))
    pb, S, _, _, _ = HR.run_setup(name, device_term(rows, table.n), mi)
    return rec, pb, S, alpha, runs, seed, after


def replay(pb, S, alpha, runs, seed, events=None):
    out = [HR.restated_run(pb, S, alpha, seed, j, events) for j in range(runs)]
    for j, r in enumerate(out):
        assert HR.pow_margin_ok(r["decisions"], alpha, r["exponents"]), f"run {j}: a pruning decision within 2^-40 of its threshold: change the seed"
    return out


def compare(rec, want, trace_run=None):
    for j, w in enumerate(want):
        assert bits([rec["score"][j]])[0] == HR.bits(w["score"]), j
        got = tuple(int(rec[key][j]) for key in ("merges", "tried", "kept", "pruned", "pairs_kept", "flags"))
        assert got == (w["merges"], w["tried"], w["kept"], w["pruned"], w["pairs_kept"], w["flags"]), j
        assert [int(x) for x in rec["masks"][j]] == w["masks"], j
    if trace_run is not None:
        w, cb = want[trace_run], HR.canonical_bits   # (a NaN's sign and payload are the machine's: hc_refs.canonical_bits)
        assert [(int(x.parent), int(x.child), cb(x.value_bits), int(x.coin)) for x in rec["merge_trace"]] == \
            [(p, c, cb(v), coin) for p, c, v, coin in w["merge_trace"]]
        assert [(int(x.cluster), int(x.connections), cb(x.value_bits), int(x.pruned)) for x in rec["prune_trace"]] == \
            [(c, k, cb(v), cut) for c, k, v, cut in w["prune_trace"]]


@pytest.mark.parametrize("name", list(HR.RUNS))
def test_runs_equal_the_restated_run_bit_for_bit(bnlib, name):
    trace_run = HR.RUNS[name][4] - 1
    rec, pb, S, alpha, runs, seed, after = run_on_device(name, trace_run=trace_run)
    events = {}
    want = replay(pb, S, alpha, runs, seed, events)
    compare(rec, want, trace_run)
    n = pb.n
    if name == "t1":
        assert all(w["merges"] == 0 and w["flags"] & HR.NO_SIMILARITY for w in want)
        assert all(bits([rec["score"][j]])[0] == HR.bits(pb.score([pb.term(0, ())], pb.k[0] - 1)) for j in range(runs))
    elif name == "t2":
        assert all(w["merges"] == 1 and not w["prune_trace"] for w in want)
    elif name == "t3":
        assert all(w["prune_trace"][0][1] == 2 for w in want)
    elif name in ("t4_mid", "n5_mid"):
        # from the DEVICE's trace counts: a run with a 0-connection visit and one with a 1-connection visit (at n = 4 no run can
        # have both: its one visit after the second merge is the only one with fewer than two) are traced again, their records counted
        seen = set()
        for kind in (0, 1):
            has = [j for j, w in enumerate(want) if kind in {v[1] for v in w["prune_trace"]}]
            assert has, f"no run of this case has a {kind}-connection visit: change the seed"
            again = run_on_device(name, trace_run=has[0])[0]
            counts = [int(x.connections) for x in again["prune_trace"]]
            assert counts.count(kind) > 0 and counts == [v[1] for v in want[has[0]]["prune_trace"]]
            assert len(counts) == sum(n - 2 - s for s in range(int(again["merges"][has[0]])))
            seen |= set(counts)
        assert {0, 1} <= seen
    elif name == "n5_alpha0":
        assert all(int(rec["pruned"][j]) == 0 and int(rec["merges"][j]) == n - 1 and int(rec["flags"][j]) & HR.ONE_CLUSTER for j in range(runs))
    elif name == "n5_alpha1":
        assert all(int(rec["pairs_kept"][j]) == 0 and int(rec["merges"][j]) == n // 2 and int(rec["flags"][j]) == HR.NO_SIMILARITY for j in range(runs))
    elif name == "t3_alpha1":
        assert all(int(rec["pairs_kept"][j]) == 0 and int(rec["merges"][j]) == 1 and int(rec["flags"][j]) == HR.NO_SIMILARITY for j in range(runs))
    elif name in ("n6_q1", "n6_q2", "n33"):
        # every merge visits |parent| * |child| candidates; fewer reached an evaluation and no term is NaN: the in-degree refusal
        sizes = {i: 1 for i in range(n)}
        w = want[trace_run]
        candidates = 0
        for s, (parent, child, _, _) in enumerate(w["merge_trace"]):
            candidates += sizes[parent] * sizes[child]
            sizes[n + s] = sizes[parent] + sizes[child]
        assert events.get("refused_nan", 0) == 0 and events["refused_q"] > 0
        assert sum(int(x) for x in rec["tried"]) == sum(x["tried"] for x in want)
        assert candidates >= int(rec["tried"][trace_run])
        assert any(int(rec["tried"][j]) < sum(a * b for a, b in _pair_sizes(n, want[j])) for j in range(runs))
    elif name == "bigk_counts":
        assert events["refused_nan"] > 0 and any(int(rec["tried"][j]) < sum(a * b for a, b in _pair_sizes(n, want[j])) for j in range(runs))
    elif name == "n64":
        assert any(m >> 32 for w in want for m in w["masks"][:32]) and any(m & 0xFFFFFFFF for w in want for m in w["masks"][32:])
        assert max(max(p, c) for w in want for p, c, _, _ in w["merge_trace"]) > 64
    elif name == "n5_zero":
        assert all(int(rec["pruned"][j]) == 0 and int(rec["merges"][j]) == n - 1 for j in range(runs))
    elif name == "n5_ties":
        first = rec["merge_trace"][0]
        assert {int(first.parent), int(first.child)} == {0, 2} and int(first.value_bits) == HR.bits(0.5)
    elif name == "n5_negative":
        assert S[0][n - 1] == -0.375 and all(w["merges"] >= 1 for w in want)
    elif name in HR.NEW_ROWS:
        # the replay over the DEVICE's terms still reaches what the row exists for (tests/test_hc_refs.py shows it over libm's)
        kind = HR.RUNS[name][6]
        assert events.get("pick_tie_gt64", 0) > 0 and events.get("pick_tie_other_lane", 0) > 0, events
        if kind == "ties":
            assert events.get("pick_tie_same_lane", 0) > 0
            if alpha > 0:
                assert all(events.get(key, 0) > 0 for key in ("pruned", "kept_pair", "visit_0", "visit_1", "visit_2")), events
            else:
                assert events["p_zero"] == events["kept_pair"] > 0 and all(int(x) == 0 for x in rec["pruned"])
        if name in HR.MAX_PARENTS:
            assert events.get("refused_q", 0) > 0 and all(bin(m).count("1") <= HR.MAX_PARENTS[name] for w in want for m in w["masks"])
        if kind in ("sparse_nonfinite", "nan_first", "inf_ties"):
            assert events.get("pick_nan_index0", 0) > 0 or alpha == 1.0
            assert events.get("pick_nan_elsewhere", 0) > 0
            if alpha == 1.0:   # pow(1, NaN) = 1: every visit prunes
                assert events["p_ge1"] == events["pruned"] > 0 and all(int(x) == 0 for x in rec["pairs_kept"])
            else:              # a NaN average: every visit keeps
                assert events["p_nan"] == events["kept_pair"] > 0 and all(int(x) == 0 for x in rec["pruned"])
                assert all(int(rec["merges"][j]) == n - 1 and int(rec["flags"][j]) == HR.ONE_CLUSTER | HR.NO_SIMILARITY for j in range(runs))
        if kind == "nan_first":
            first = rec["merge_trace"][0]
            assert {int(first.parent), int(first.child)} == {0, 1} and HR.canonical_bits(first.value_bits) == HR.bits(math.nan)
        if kind == "inf_ties":
            first, second = rec["merge_trace"][0], rec["merge_trace"][1]
            assert {int(first.parent), int(first.child)} == set(HR.INF_TIES_PAIRS[0]) and int(first.value_bits) == HR.bits(math.inf)
            assert {int(second.parent), int(second.child)} == set(HR.INF_TIES_NAN) and HR.canonical_bits(second.value_bits) == HR.bits(math.nan)
        if kind == "inf_sparse":
            assert all(events.get(key, 0) > 0 for key in ("p_nan", "p_ge1", "p_zero", "pruned", "kept_pair", "visit_0", "visit_1", "visit_2")), events
    # the winner: the strictly smallest score, the lowest run among equals; the learner holds its graph and terms
    scores = [w["score"] for w in want]
    winner = scores.index(min(scores))
    assert rec["winner"] == winner
    score, (ll, params), parents, n_runs, n_merges, ns = after
    assert bits([score])[0] == HR.bits(want[winner]["score"])
    assert score == LR.score_arith(ll, params, pb.criterion, pb.total)
    assert np.array_equal(bits(ll), bits(want[winner]["ll"])) and params == want[winner]["params"]
    assert parents == [list(AR._parents_of(m)) for m in want[winner]["masks"]]
    assert n_runs == runs and n_merges == sum(w["merges"] for w in want) and ns > 0


def _pair_sizes(n, w):
    sizes = {i: 1 for i in range(n)}
    out = []
    for s, (parent, child, _, _) in enumerate(w["merge_trace"]):
        out.append((sizes[parent], sizes[child]))
        sizes[n + s] = sizes[parent] + sizes[child]
    return out


def test_a_run_does_not_depend_on_the_number_of_runs(bnlib):
    full = run_on_device("n5_mid")[0]
    for runs in (1, 5):
        part = run_on_device("n5_mid", runs=runs)[0]
        for key in ("score", "merges", "tried", "kept", "pruned", "pairs_kept", "flags", "masks"):
            assert np.array_equal(np.asarray(part[key]).view(np.uint8), np.asarray(full[key][:runs]).view(np.uint8)), (runs, key)


def test_among_equal_scores_the_lowest_run_wins(bnlib):
    """n = 2, alpha = 0, a caller's symmetric matrix: a run is its coin, so runs with equal coins are identical runs."""
    rec, pb, S, alpha, runs, seed, _ = run_on_device("t2_tie")
    best = rec["score"].min()
    ties = [j for j in range(runs) if bits([rec["score"][j]])[0] == bits([best])[0]]
    assert len(ties) >= 2 and rec["winner"] == ties[0]
    assert [int(x) for x in rec["masks"][ties[0]]] == [int(x) for x in rec["masks"][ties[1]]]


def test_a_matrix_whose_triangles_differ_in_bits_is_refused(bnlib):
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = HR.hc_input("n5")
    with info_table(table) as t, TermTable(t, 2) as tt, Learner(t, None, "aic") as L:
        S = HR.similarity_matrix("negative", 5).copy()
        S[1][3] = np.nextafter(S[1][3], 1.0)
        with pytest.raises(_lib.BnError) as ei:
            L.hc(tt, 0.5, 4, 1, similarity=S)
        assert ei.value.code == _lib.BN_ERR_ARG and "[1][3]" in str(ei.value) and L.info("hc_runs") == 0
        S = HR.similarity_matrix("zero", 5).copy()
        S[2][4] = -0.0                                          # equal as numbers, not in bits
        with pytest.raises(_lib.BnError) as ei:
            L.hc(tt, 0.5, 4, 1, similarity=S)
        assert ei.value.code == _lib.BN_ERR_ARG and L.info("hc_runs") == 0
        S = HR.similarity_matrix("negative", 5).copy()
        S[0][0] = math.nan                                      # the diagonal is not read
        L.hc(tt, 0.5, 4, 1, similarity=S)
        assert L.info("hc_runs") == 4


def test_the_learned_graph_scores_the_same_through_the_public_api(bnlib):
    from bayesiannetwork_amd.engine import Engine, fit_cpt
    from bayesiannetwork_amd.evaluation import AIC, MDL
    from bayesiannetwork_amd.learning import Learner, TermTable, structure_model
    _, table = AR.anneal_input("n33")
    with info_table(table) as t, TermTable(t, 3) as tt:
        for criterion, ev in (("aic", AIC(t)), ("mdl", MDL(t))):
            with Learner(t, None, criterion) as L:
                empty = L.score()
                L.hc(tt, 0.3, runs=16, seed=21)
                ptr, idx = L.structure()
                m = structure_model(table.k, ptr, idx)
                m.cpt[:] = fit_cpt(m, table.pats, table.counts, device=0)
                with Engine(m, device=0) as eng:
                    diff, B = abs(L.score() - ev(eng)), LR.graph_bound(table, L.parents(), criterion)
                print(f"{criterion}: {len(idx)} edges, score {L.score():.6f} (empty {empty:.6f}); |score - public score| = {diff:.3g}, B = {B:.3g}")
                assert diff <= B and L.score() < empty and all(len(p) <= 3 for p in L.parents())


def test_stepwise_structure_hc_end_to_end(bnlib):
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import MDL
    from bayesiannetwork_amd.learning import BruteForce, Learner, StepwiseStructureHC, structure_model
    model, table, criterion, _, _ = LR.learning_input("alarm2k_mdl")
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table) as t:
        with Learner(t, None, "mdl") as L0:
            empty = L0.score()
        hc = StepwiseStructureHC("mdl", t, max_parents=3, runs=64, seed=5)
        learned, score = hc(start, 0.3)
        learned.validate()                                            # a DAG with CPTs of the right shape
        parents = [learned.parents(v).tolist() for v in range(model.n)]
        assert all(len(p) <= 3 for p in parents) and sum(map(len, parents)) > 0 and score < empty
        with Learner(t, learned, "mdl") as L1:
            assert L1.score() == score
        with Engine(learned, device=0) as eng:
            assert abs(MDL(t)(eng) - score) <= LR.graph_bound(table, parents, "mdl")
        first = dict(hc.last)
        assert first["term_entries"] == 37 * 7807 and first["hc_runs"] == 64 and first["hc_merges"] >= 64 and 0 <= first["winner"] < 64
        again, score2 = hc(start, 0.3)
        assert hc.last["term_passes"] == first["term_passes"] and hc.last["term_families_scored"] == first["term_families_scored"]
        assert score2 < empty
        hc.close()
    _, table6 = AR.anneal_input("n6")
    with info_table(table6) as t6:
        with Learner(t6, None, "aic") as L0:
            empty6 = L0.score()
        host = StepwiseStructureHC("aic", t6, between=BruteForce, seed=3)
        m6 = structure_model(table6.k, np.zeros(7, np.int32), np.zeros(0, np.int32))
        learned6, score6 = host(m6, 0.2)
        learned6.validate()
        assert score6 <= empty6 and host.last["hc_runs"] == 1 and host.last["hc_merges"] >= 1 and host.records is None


def test_argument_errors_launch_nothing(bnlib):
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = AR.anneal_input("n5")
    with info_table(table) as t, info_table(table) as other, TermTable(t, 2) as tt, TermTable(other, 2) as tt_other:
        with Learner(t, [[], [0], [], [], [0, 1, 2]], "aic") as L:     # the starting edges are ignored, whatever they are
            for bad in (dict(alpha=-0.5), dict(alpha=math.inf), dict(alpha=math.nan), dict(runs=0), dict(runs=(1 << 16) + 1),
                        dict(max_parents=3), dict(max_parents=0), dict(trace_run=4), dict(trace_run=-2)):
                with pytest.raises(_lib.BnError) as ei:
                    L.hc(tt, **{**dict(alpha=0.5, runs=4), **bad})
                assert ei.value.code == _lib.BN_ERR_ARG, bad
            with pytest.raises(_lib.BnError) as ei:
                L.hc(tt_other, 0.5, 4)
            assert ei.value.code == _lib.BN_ERR_ARG
            with pytest.raises(ValueError):
                L.hc(tt, 0.5, 4, similarity=np.zeros((4, 4)))
            assert L.info("hc_runs") == 0 and L.info("hc_merges") == 0 and L.info("edges") == 4
            rec = L.hc(tt, 0.5, 4, 9)
            with Learner(t, None, "aic") as clean:
                ref = clean.hc(tt, 0.5, 4, 9)
            assert np.array_equal(bits(rec["score"]), bits(ref["score"])) and np.array_equal(rec["masks"], ref["masks"])
