"""Simulated annealing on the GPU (bn_terms_*, bn_learn_anneal of include/bn_mi355x.h; bayesiannetwork_amd.learning.TermTable,
Learner.anneal, SimulatedAnnealing) against tests/anneal_refs.py.

The term table is compared bit for bit with bn_learn_score_groups at the restated rank.  Chains are compared bit for bit with the
restated chain (which tests/test_anneal_refs.py holds equal to the literal transcription of the reference's loop) replayed over
the DEVICE's own fetched terms: every arithmetic step but exp is then the same on both sides, and before any comparison the replay
shows that no uphill decision is within 2^-40 (relative) of its threshold -- none is left out."""
import math
from math import comb

import numpy as np
import pytest

import anneal_refs as AR
import learning_refs as LR
from bayesiannetwork_amd import _lib

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def info_table(table):
    from bayesiannetwork_amd.evaluation import InfoTable
    return InfoTable(table.pats, table.counts, table.k, device=0)


def restated_rank(n, child, parents):
    """The header's index, restated: s' = s - (s > child); offset[j] + sum_i C(s'_i, i)."""
    ps = sorted(parents)
    return sum(comb(n - 1, t) for t in range(len(ps))) + sum(comb(s - (s > child), i + 1) for i, s in enumerate(ps))


def device_term(rows, n):
    """term(child, parents) over the fetched rows of a TermTable."""
    return lambda child, parents: float(rows[child][restated_rank(n, child, parents)])


# ---- the term table ----------------------------------------------------------------------------------

def check_entries(t, table, tt, q, families):
    """Every (child, parents) of `families`: the entry at the restated rank has the bits score_groups gives the family."""
    from bayesiannetwork_amd.learning import score_groups
    n = table.n
    rows = {c: tt.row(c) for c in {c for c, _ in families}}
    want = score_groups(t, [(c, list(S), []) for c, S in families])
    for (c, S), w in zip(families, want):
        assert tt.rank(c, S) == restated_rank(n, c, S) == AR.rank(n, c, S)
        assert bits([rows[c][restated_rank(n, c, S)]])[0] == bits(w)[0], (c, S)


def test_term_table_n6_every_subset_mixed_arities(bnlib):
    from bayesiannetwork_amd.learning import TermTable
    _, table = AR.anneal_input("n6")   # arities 2, 1, 3, 4, 2, 5
    n, q = 6, 5
    with info_table(table) as t, TermTable(t, q) as tt:
        T = AR.row_entries(n, q)
        assert (tt.row_entries, tt.info("entries"), tt.info("nodes"), tt.info("max_parents")) == (T, n * T, n, q)
        assert T == 2 ** 5 and tt.info("ineligible") == 0 and tt.info("families_scored") >= n * T and tt.info("build_ns") > 0
        families = [(c, AR.unrank(n, q, c, r)) for c in range(n) for r in range(T)]
        assert len({(c, tuple(S)) for c, S in families}) == n * T
        check_entries(t, table, tt, q, families)


@pytest.mark.parametrize("name,q", [("n33", 3), ("n64", 2), ("n64", 3)])
def test_term_table_sampled_entries(bnlib, name, q):
    from bayesiannetwork_amd.learning import TermTable
    _, table = AR.anneal_input(name)
    n = table.n
    T = AR.row_entries(n, q)
    rng = np.random.default_rng(n)
    picks = set()
    edges = [0] + [sum(comb(n - 1, t) for t in range(j + 1)) for j in range(q + 1)]   # the size classes' boundaries
    for c in (0, 1, 31, 32, n - 1):
        for j in range(q + 1):
            picks.add((c, edges[j]))            # the first and the last of each size class
            picks.add((c, edges[j + 1] - 1))
    for hi in (31, 32, 63):                     # sets that contain nodes 31, 32 and 63
        if hi < n:
            for c in (0, 30, 33 % n):
                others = [u for u in range(n) if u not in (c, hi)]
                for j in range(q):
                    for _ in range(20):
                        S = sorted([hi] + [int(x) for x in rng.choice(others, j, replace=False)])
                        picks.add((c, AR.rank(n, c, S)))
    while len(picks) < 1100:
        picks.add((int(rng.integers(n)), int(rng.integers(T))))
    families = [(c, AR.unrank(n, q, c, r)) for c, r in sorted(picks)]
    assert len(families) >= 1000 and any(31 in S for _, S in families) and any(32 in S for _, S in families)
    assert name != "n64" or any(63 in S for _, S in families)
    with info_table(table) as t, TermTable(t, q) as tt:
        assert tt.row_entries == T and tt.info("ineligible") == 0
        check_entries(t, table, tt, q, families)


def test_a_family_over_the_limit_is_nan_and_the_size_limits_are_named(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import TermTable
    _, table = AR.anneal_input("bigk")   # arities 255, 255, 255, 2
    n, q = 4, 3
    with info_table(table) as t, TermTable(t, q) as tt:
        T = AR.row_entries(n, q)
        nan = 0
        for c in range(n):
            row = tt.row(c)
            for r in range(T):
                S = AR.unrank(n, q, c, r)
                over = int(table.k[c]) * math.prod(int(table.k[u]) for u in S) > (1 << 20)
                assert math.isnan(row[r]) == over, (c, S)
                nan += over
        assert nan > 0 and tt.info("ineligible") == nan
        check_entries(t, table, tt, q, [(c, S) for c in range(n) for S in ([], [(c + 1) % n]) ])
        with pytest.raises(_lib.BnError) as ei:
            TermTable(t, 0)
        assert ei.value.code == _lib.BN_ERR_ARG
        with pytest.raises(_lib.BnError) as ei:
            TermTable(t, 17)
        assert ei.value.code == _lib.BN_ERR_ARG
    pats = np.zeros((3, 65), np.uint8)
    pats[1, :] = 1
    with InfoTable(pats, np.ones(3, np.uint64), [2] * 65, device=0) as t65:
        with pytest.raises(_lib.BnError) as ei:
            TermTable(t65, 1)
        assert ei.value.code == _lib.BN_ERR_ARG and "65" in str(ei.value) and "64" in str(ei.value)
    with InfoTable(pats[:, :64], np.ones(3, np.uint64), [2] * 64, device=0) as t64:
        with pytest.raises(_lib.BnError) as ei:
            TermTable(t64, 4)                      # 64 * T(64, 4) = 64 * 637 393
        assert ei.value.code == _lib.BN_ERR_ARG and str(64 * AR.row_entries(64, 4)) in str(ei.value) and str(1 << 22) in str(ei.value)


# ---- chains, bit for bit ---------------------------------------------------------------------------------

def run_on_device(name, chains=None, trace_chain=None):
    """(device records, Problem over the device's terms, Schedule, chains, seed, score after, terms after, parents after)."""
    from bayesiannetwork_amd.learning import Learner, TermTable
    inp, q, criterion, rule, t0, t1, rate, boltz, same, cap, n_chains, seed, start = AR.RUNS[name]
    chains = n_chains if chains is None else chains
    _, table = AR.anneal_input(inp)
    with info_table(table) as t, TermTable(t, q) as tt:
        rows = [tt.row(c) for c in range(table.n)]
        bound = {"max_parents": AR.MAX_PARENTS[name]} if name in AR.MAX_PARENTS else {}   # (below the table's q)
        with Learner(t, start, criterion, **bound) as L:
            rec = L.anneal(tt, t0, t1, rate, boltz, same, chains, seed, rule, cap, trace_chain=trace_chain)
            after = (L.score(), L.terms(), L.parents(), L.info("anneal_chains"), L.info("anneal_steps"), L.info("anneal_ns"))
    pb, sched, _, _ = AR.run_setup(name, device_term(rows, table.n))
    return rec, pb, sched, chains, seed, after


def replay(pb, sched, chains, seed, events=None):
    """The restated chains over the device's terms; the exp margin is checked on EVERY uphill decision before anything is compared."""
    out = [AR.restated_chain(pb, sched, seed, j, events) for j in range(chains)]
    for j, r in enumerate(out):
        assert AR.exp_margin_ok(r["uphill"]), f"chain {j}: an uphill decision within 2^-40 of its threshold: change the seed"
    return out


def compare(rec, want, trace_chain=None):
    for j, w in enumerate(want):
        assert bits([rec["eval"][j]])[0] == AR.bits(w["eval"]), j
        got = (int(rec["proposals"][j]), int(rec["operated"][j]), int(rec["accepted"][j]), int(rec["flags"][j]))
        assert got == (w["proposals"], w["operated"], w["accepted"], w["flags"]), j
        assert [int(x) for x in rec["masks"][j]] == w["masks"], j
        assert rec["edges"][j] == [tuple(e) for e in w["edges"]], j
    if trace_chain is not None:
        tr = rec["trace"]
        got = [(int(x["method"]), int(x["from"]), int(x["to"]), int(x["now_bits"]), bool(x["accepted"])) for x in tr]
        assert got == want[trace_chain]["trace"]


@pytest.mark.parametrize("name", list(AR.RUNS))
def test_chains_equal_the_restated_chain_bit_for_bit(bnlib, name):
    trace_chain = AR.RUNS[name][10] - 1 if AR.RUNS[name][10] < 100 else 129
    rec, pb, sched, chains, seed, after = run_on_device(name, trace_chain=trace_chain)
    events = {}
    want = replay(pb, sched, chains, seed, events)
    compare(rec, want, trace_chain)
    if name in ("n64_dense_met", "n64_dense_ref"):
        # over the DEVICE's terms the chains still hold the long list and erase, accept and reject in it 64 entries at a time
        assert all(events.get(key, 0) > 0 for key in ("erase_tail_gt64", "erase_tail_gt128", "copy_gt64_accept", "copy_gt64_reject",
                                                      "reverse_refused_moved_gt64")), events
        assert max(w["longest_list"] for w in want) >= 180
    elif name == "n33_dense_ref":
        assert all(events.get(key, 0) > 0 for key in ("erase_tail_gt64", "copy_gt64_accept", "copy_gt64_reject")), events
    elif name == "n33_bound2_over_q3":
        assert events.get("refused_q", 0) > 0 and all(bin(m).count("1") <= 2 for w in want for m in w["masks"])
    elif name in ("n5_long_met", "n6_long_ref"):
        assert all(w["flags"] == AR.END_TEMPERATURE and w["proposals"] > 10000 for w in want)
    # the winner: the strictly smallest evaluation, the lowest index among equals; the learner holds its graph and terms
    evals = [w["eval"] for w in want]
    winner = evals.index(min(evals))
    assert rec["winner"] == winner
    score, (ll, params), parents, n_chains, n_steps, ns = after
    assert bits([score])[0] == AR.bits(want[winner]["eval"])
    assert score == LR.score_arith(ll, params, pb.criterion, pb.total)
    assert np.array_equal(bits(ll), bits(want[winner]["ll"])) and params == want[winner]["params"]
    assert parents == [list(AR._parents_of(m)) for m in want[winner]["masks"]]
    assert n_chains == chains and n_steps == sum(w["proposals"] for w in want) and ns > 0


def test_the_flags_say_how_a_chain_ended(bnlib):
    for name, flag in (("n1_cap", AR.END_CAP), ("n5_cap", AR.END_CAP), ("n5_same_state", AR.END_SAME_STATE), ("n5_met_aic", AR.END_TEMPERATURE)):
        rec = run_on_device(name)[0]
        assert all(int(f) == flag for f in rec["flags"]), (name, rec["flags"])
    rec = run_on_device("n1_cap")[0]
    assert int(rec["proposals"][0]) == 50 and int(rec["operated"][0]) == 0 and rec["edges"][0] == []


def test_a_chain_does_not_depend_on_the_number_of_chains(bnlib):
    full = run_on_device("n33_met_aic")[0]
    for chains in (1, 5):
        part = run_on_device("n33_met_aic", chains=chains)[0]
        for key in ("eval", "proposals", "operated", "accepted", "flags", "masks"):
            assert np.array_equal(np.asarray(part[key]).view(np.uint8), np.asarray(full[key][:chains]).view(np.uint8)), (chains, key)
        assert part["edges"] == full["edges"][:chains]


def test_among_equal_evaluations_the_lowest_chain_wins(bnlib):
    """n = 2, two iterations per chain: seed 26 leaves chain 0 without an edge and ends chains 2 and 3 in the same, best graph --
    two identical chains, so two evaluations with the same bits."""
    rec = run_on_device("n2_tie")[0]
    best = rec["eval"].min()
    ties = [j for j in range(8) if rec["eval"][j] == best]
    assert ties[:2] == [2, 3] and rec["winner"] == 2 and rec["eval"][0] > best
    assert [int(x) for x in rec["masks"][2]] == [int(x) for x in rec["masks"][3]] == [2, 0]


def test_the_learned_graph_scores_the_same_through_the_public_api(bnlib):
    from bayesiannetwork_amd.engine import Engine, fit_cpt
    from bayesiannetwork_amd.evaluation import AIC, MDL
    from bayesiannetwork_amd.learning import Learner, TermTable, structure_model
    _, table = AR.anneal_input("n33")
    with info_table(table) as t, TermTable(t, 3) as tt:
        for criterion, ev in (("aic", AIC(t)), ("mdl", MDL(t))):
            with Learner(t, None, criterion) as L:
                empty = L.score()
                L.anneal(tt, 20.0, 0.2, 0.9, chains=16, seed=21, rule="metropolis")
                ptr, idx = L.structure()
                m = structure_model(table.k, ptr, idx)
                m.cpt[:] = fit_cpt(m, table.pats, table.counts, device=0)
                with Engine(m, device=0) as eng:
                    diff, B = abs(L.score() - ev(eng)), LR.graph_bound(table, L.parents(), criterion)
                print(f"{criterion}: {len(idx)} edges, score {L.score():.6f} (empty {empty:.6f}); |score - public score| = {diff:.3g}, B = {B:.3g}")
                assert diff <= B and L.score() < empty and all(len(p) <= 3 for p in L.parents())


def test_simulated_annealing_end_to_end(bnlib):
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import MDL
    from bayesiannetwork_amd.learning import Learner, SimulatedAnnealing, structure_model
    model, table, criterion, _, _ = LR.learning_input("alarm2k_mdl")
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table) as t:
        sa = SimulatedAnnealing("mdl", t, max_parents=3, chains=64, rule="metropolis", seed=5)
        learned, score = sa(start, 20.0, 0.5, 0.95)
        learned.validate()                                            # a DAG with CPTs of the right shape
        parents = [learned.parents(v).tolist() for v in range(model.n)]
        assert all(len(p) <= 3 for p in parents) and sum(map(len, parents)) > 0
        with Learner(t, None, "mdl") as L0, Learner(t, learned, "mdl") as L1:
            assert score <= L0.score() and L1.score() == score
        with Engine(learned, device=0) as eng:
            assert abs(MDL(t)(eng) - score) <= LR.graph_bound(table, parents, "mdl")
        first = dict(sa.last)
        assert first["term_entries"] == 37 * 7807 and first["anneal_chains"] == 64 and first["anneal_steps"] > 64 and 0 <= first["winner"] < 64
        again, score2 = sa(start, 20.0, 0.5, 0.95)
        assert sa.last["term_passes"] == first["term_passes"] and sa.last["term_families_scored"] == first["term_families_scored"]
        assert score2 <= L0_score(t)
        sa.close()
        ref = SimulatedAnnealing("mdl", t, seed=5)                   # the defaults: q = 3, 64 chains, the reference's rule
        _, score3 = ref(start, 1e6, 1e4, 0.9)
        assert score3 <= L0_score(t) and ref.last["anneal_chains"] == 64
        ref.close()


def L0_score(t):
    from bayesiannetwork_amd.learning import Learner
    with Learner(t, None, "mdl") as L0:
        return L0.score()


def test_argument_errors_launch_nothing(bnlib):
    from bayesiannetwork_amd.learning import Learner, TermTable
    _, table = AR.anneal_input("n5")
    with info_table(table) as t, info_table(table) as other, TermTable(t, 2) as tt, TermTable(other, 2) as tt_other:
        with Learner(t, None, "aic") as L:
            good = dict(initial_temp=10.0, final_temp=1.0, decreasing_rate=0.9)
            for bad in (dict(decreasing_rate=1.0), dict(decreasing_rate=1.5), dict(decreasing_rate=0.0), dict(initial_temp=0.0),
                        dict(final_temp=-1.0), dict(initial_temp=math.inf), dict(final_temp=math.nan), dict(boltzmann=0.0), dict(chains=0),
                        dict(chains=(1 << 16) + 1), dict(max_proposals=(1 << 24) + 1), dict(trace_chain=64)):
                with pytest.raises(_lib.BnError) as ei:
                    L.anneal(tt, **{**good, **bad})
                assert ei.value.code == _lib.BN_ERR_ARG, bad
            with pytest.raises(_lib.BnError) as ei:
                L.anneal(tt_other, **good)
            assert ei.value.code == _lib.BN_ERR_ARG
            with pytest.raises(ValueError):
                L.anneal(tt, rule="other", **good)
            assert L.info("anneal_chains") == 0 and L.info("anneal_steps") == 0 and L.info("edges") == 0
        with Learner(t, [[], [], [], [], [0, 1, 2]], "aic") as L:      # a starting family over q = 2
            with pytest.raises(_lib.BnError) as ei:
                L.anneal(tt, **good)
            assert ei.value.code == _lib.BN_ERR_ARG and "3 parents" in str(ei.value) and L.info("anneal_chains") == 0
