"""Bayesian-Dirichlet scores on the GPU (bn_score_spec, bn_*_spec of include/bn_mi355x.h; BDeu / K2Score of
bayesiannetwork_amd.evaluation and every search of bayesiannetwork_amd.learning under them) against tests/bd_refs.py.

Counts are compared exactly.  A family term is compared bit for bit with itself across groupings, positions, splits, the subset
lattice and the term table, and with math.fsum of the restated terms through B_bd = (26u + gamma_{m+1}) * sum M.
The searches are compared with the host loops over the RESTATED terms on the inputs whose every decision tests/test_bd_refs.py
shows to have a margin of more than 1000 bounds -- equal edges, no decision left out -- and bit for bit with the same loops over
the DEVICE's own terms.  The full brute-force enumeration under BDeu is the one search whose decisions cannot have a margin (score
equivalence, shown in tests/test_bd_refs.py): it is held to the loop over the device's terms bit for bit and to the restated best
score within the bounds; under K2 its edges are demanded as everywhere else."""
import ctypes
import math

import numpy as np
import pytest

import anneal_refs as AR
import bd_refs as BD
import hc_refs as HR
import learning_refs as LR
from bayesiannetwork_amd import _lib

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def info_table(pats, counts, k):
    from bayesiannetwork_amd.evaluation import InfoTable
    return InfoTable(pats, counts, k, device=0)


def flat(lists):
    return [x for row in lists for x in row]


# ---- terms: exact counts, the bound against the restatement ----------------------------------------------

@pytest.mark.parametrize("P,specs", BD.TERM_CASES, ids=lambda x: str(x) if isinstance(x, int) else "")
def test_counts_are_exact_and_terms_are_within_the_bound(bnlib, P, specs):
    from bayesiannetwork_amd.learning import score_groups
    pats, counts = BD.term_table(P)
    families = list(BD.families_of(BD.GROUPS))
    want_N = [LR.family_counts(pats, counts, BD.KS, c, ps) for c, ps in families]
    with info_table(pats, counts, BD.KS) as t:
        for spec in specs:
            bd, N = score_groups(t, BD.GROUPS, counts=True, criterion=spec.criterion())
            worst = 0.0
            for (child, parents), got, got_N, w_N in zip(families, flat(bd), flat(N), want_N):
                assert np.array_equal(got_N, w_N), (child, parents)
                _, exact, bound = BD.bd_family(w_N, BD.KS[child], spec)
                err = abs(got - exact)
                worst = max(worst, err / bound if bound else 0.0)
                assert err <= bound, (spec, child, parents, err, bound)
                if BD.KS[child] == 1:
                    assert bound > 0.0 or got == 0.0          # an arity-1 child: log 1, within its bound of 0
            print(f"P = {P}, {spec}: largest |bd - fsum| / B_bd over {len(families)} families: {worst:.3g}")


def test_small_counts_and_an_all_zero_row(bnlib):
    """Counts 0, 1, 15, 16, 17 (a_c + N exactly 16 under K2) and a parent state no sample shows."""
    from bayesiannetwork_amd.learning import score_groups
    with info_table(BD.SMALL_PATS, BD.SMALL_COUNTS, BD.SMALL_K) as t:
        for spec in BD.SPECS:
            bd, N = score_groups(t, [(1, [0], [])], counts=True, criterion=spec.criterion())
            assert N[0][0].tolist() == [0, 1, 15, 16, 17, 0, 0, 0]
            _, exact, bound = BD.bd_family(N[0][0], 2, spec)
            assert abs(bd[0][0] - exact) <= bound and bd[0][0] < 0.0, spec


# ---- a term is a function of the counts and the spec ------------------------------------------------------

@pytest.mark.parametrize("spec", [BD.BDEU10, BD.K2S], ids=repr)
def test_terms_have_the_same_bits_everywhere(bnlib, spec):
    from bayesiannetwork_amd.learning import score_groups, score_subsets
    crit = spec.criterion()
    P = 4097
    pats, counts = BD.term_table(P)
    with info_table(pats, counts, BD.KS) as t:
        bd = score_groups(t, BD.GROUPS, criterion=crit)
        by_family = {(c, tuple(p)): x for (c, p), x in zip(BD.families_of(BD.GROUPS), flat(bd))}
        for splits in (1, 2, 7):
            assert np.array_equal(bits(flat(score_groups(t, BD.GROUPS, splits=splits, criterion=crit))), bits(flat(bd))), splits
        alone = [(c, p, []) for c, p in BD.families_of(BD.GROUPS)]                 # every family as the base of its own group
        assert np.array_equal(bits([score_groups(t, [g], criterion=crit)[0][0] for g in alone]), bits(flat(bd)))
        assert np.array_equal(bits(flat(score_groups(t, alone, criterion=crit))), bits(flat(bd)))
        permuted = [(c, b, list(reversed(us))) for c, b, us in reversed(BD.GROUPS)]
        for (c, p), x in zip(BD.families_of(permuted), flat(score_groups(t, permuted, criterion=crit))):
            assert bits([x])[0] == bits([by_family[(c, tuple(p))]])[0], (c, p)
        want = by_family[(17, (3, 5, 9, 28))]                                     # as a candidate of other bases
        for base, u in (([5, 9, 28], 3), ([3, 5, 9], 28), ([3, 5, 28], 9)):
            assert bits([score_groups(t, [(17, base, [0, u])], criterion=crit)[0][2]])[0] == bits([want])[0]
        # the subset lattice: the LDS form (top family 3 * 2 * 4 * 2 * 5 = 240 cells) and the per-level form (16^3 * 2 = 8 192)
        for child, base, cand in ((17, [28], [0, 3, 29]), (25, [23], [24, 0])):
            got = score_subsets(t, child, base, cand, criterion=crit)
            fams = [(child, sorted(base + [cand[j] for j in range(len(cand)) if (mask >> j) & 1]), []) for mask in range(1 << len(cand))]
            assert np.array_equal(bits(got), bits(flat(score_groups(t, fams, criterion=crit)))), (child, base, cand)
            for splits in (1, 7):
                assert np.array_equal(bits(score_subsets(t, child, base, cand, splits=splits, criterion=crit)), bits(got))
    # the same samples as other rows
    order = np.random.default_rng(5).permutation(P)
    with info_table(pats[order], counts[order], BD.KS) as t:
        assert np.array_equal(bits(flat(score_groups(t, BD.GROUPS, criterion=crit))), bits(flat(bd)))


def test_kind_zero_through_the_spec_entry_points_has_the_old_bits(bnlib):
    from bayesiannetwork_amd.learning import Learner, TermTable, score_groups, score_subsets
    pats, counts = BD.term_table(2049)
    with info_table(pats, counts, BD.KS) as t:
        assert np.array_equal(bits(flat(score_groups(t, BD.GROUPS, criterion="aic"))), bits(flat(score_groups(t, BD.GROUPS))))
        a, Na = score_subsets(t, 17, [28], [0, 3, 29], counts=True, criterion="mdl")
        b, Nb = score_subsets(t, 17, [28], [0, 3, 29], counts=True)
        assert np.array_equal(bits(a), bits(b)) and all(np.array_equal(x, y) for x, y in zip(Na, Nb))
        # bn_learn_create_spec / bn_terms_create_spec with a kind-0 spec and with NULL
        lib, spec0 = _lib.lib(), _lib.ScoreSpec(0, 0, 7.0)
        one = np.zeros(len(BD.KS) + 1, np.int32)
        p32 = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        with Learner(t, None, "mdl") as L:
            for sp in (ctypes.byref(spec0), None):
                h, s = ctypes.c_void_p(), ctypes.c_double()
                _lib.check(lib.bn_learn_create_spec(t._h, p32(one), None, 1, sp, 16, ctypes.byref(h)))
                _lib.check(lib.bn_learn_score(h, ctypes.byref(s)))
                lib.bn_learn_destroy(h)
                assert bits([s.value])[0] == bits([L.score()])[0] and L.info("criterion") == 1
    _, table = AR.anneal_input("n5")
    with info_table(table.pats, table.counts, table.k) as t, TermTable(t, 2) as old, TermTable(t, 2, "aic") as new:
        assert all(np.array_equal(bits(old.row(c)), bits(new.row(c))) for c in range(5))
        assert (new.info("score_kind"), new.info("ess_bits")) == (0, 0) and old.spec == new.spec == (0, 0.0)


@pytest.mark.parametrize("spec", [BD.BDEU_HALF, BD.K2S], ids=repr)
@pytest.mark.parametrize("name,q", [("n6", 5), ("n33", 3)])
def test_term_table_entries_are_the_group_scores_at_the_restated_rank(bnlib, name, q, spec):
    from bayesiannetwork_amd.learning import TermTable, score_groups
    crit = spec.criterion()
    _, table = AR.anneal_input(name)
    n, T = table.n, AR.row_entries(table.n, q)
    if name == "n6":
        families = [(c, AR.unrank(n, q, c, r)) for c in range(n) for r in range(T)]      # every subset, arities 2, 1, 3, 4, 2, 5
    else:
        rng = np.random.default_rng(33)
        picks = {(c, r) for c in (0, 31, 32) for r in (0, 1, T - 1)}
        while len(picks) < 300:
            picks.add((int(rng.integers(n)), int(rng.integers(T))))
        families = [(c, AR.unrank(n, q, c, r)) for c, r in sorted(picks)]
    with info_table(table.pats, table.counts, table.k) as t, TermTable(t, q, crit) as tt:
        assert tt.row_entries == T and tt.info("score_kind") == spec.kind and tt.info("ess_bits") == int(bits([spec.ess])[0])
        rows = {c: tt.row(c) for c in {c for c, _ in families}}
        want = score_groups(t, [(c, list(S), []) for c, S in families], criterion=crit)
        for (c, S), w in zip(families, want):
            assert bits([rows[c][AR.rank(n, c, S)]])[0] == bits(w)[0], (c, S)


# ---- properties ------------------------------------------------------------------------------------------------

def test_bdeu_is_score_equivalent_and_an_arity_one_family_scores_zero(bnlib):
    from bayesiannetwork_amd.evaluation import BDeu
    from bayesiannetwork_amd.learning import Learner, score_groups
    _, table = AR.anneal_input("n6")   # arities 2, 1, 3, 4, 2, 5
    for spec in (BD.BDEU1, BD.BDEU10):
        bdt = BD.BDTable(table, spec)
        with info_table(table.pats, table.counts, table.k) as t:
            totals = []
            for parents in ([[], [], [0], [2], [], []], [[2], [], [3], [], [], []], [[2], [], [], [2], [], []]):   # 0->2->3, 0<-2<-3, 0<-2->3
                with Learner(t, parents, BDeu(spec.ess)) as L:
                    totals.append((L.score(), bdt.graph_bound(parents)))
            for (a, Ba), (b, Bb) in ((totals[0], totals[1]), (totals[0], totals[2])):
                assert a != 0.0 and abs(a - b) <= Ba + Bb, (spec, a, b, Ba + Bb)
            one = score_groups(t, [(1, [], [0, 3])], criterion=spec.criterion())[0]
            for x, ps in zip(one, ([], [0], [3])):
                assert abs(x) <= bdt.family(1, ps)[2], (spec, ps, x)


# ---- the searches ----------------------------------------------------------------------------------------------------

def device_term(t, crit):
    from bayesiannetwork_amd.learning import score_groups
    cache = {}

    def term(child, parents):
        key = (child, tuple(sorted(parents)))
        if key not in cache:
            cache[key] = score_groups(t, [(child, list(key[1]), [])], criterion=crit)[0][0]
        return cache[key]
    return term


def as_lists(out):
    return {name: (flags, parents) for name, (flags, parents, _) in out.items() if name != "margins"}


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
def test_greedy_hint_k2_and_best_parents(bnlib, spec):
    """Equal edges with the host loops over the restated terms (margins: tests/test_bd_refs.py), the final score within the graph's
    bound; and the scan IS the sequential loop over the device's own terms, bit for bit."""
    from bayesiannetwork_amd.learning import Learner
    crit = spec.criterion()
    model, table = BD.learner_input()
    bdt = BD.BDTable(table, spec)
    with info_table(table.pats, table.counts, model.k) as t:
        learners = []

        def make(start):
            learners.append(Learner(t, start, crit, BD.MAX_PARENTS))
            return learners[-1]

        got = BD.run_searches(make)
        restated = BD.run_searches(lambda start: BD.BDSearch(model.k, start, bdt.term, BD.MAX_PARENTS))
        own = BD.run_searches(lambda start: BD.BDSearch(model.k, start, device_term(t, crit), BD.MAX_PARENTS))
        for name in ("greedy", "hint", "k2", "best"):
            flags, parents, L = got[name]
            assert flags == restated[name][0] and parents == restated[name][1], name
            assert sum(map(len, parents)) > 0 and L.info("criterion") == spec.kind
            assert abs(L.score() - restated[name][2].score) <= bdt.graph_bound(parents), name
            assert flags == own[name][0] and bits([L.score()])[0] == bits([own[name][2].score])[0], name
            ll, params = L.terms()
            assert L.score() == BD.likelihood_alone(ll) and params == sum(LR.family_params(model.k, v, p) for v, p in enumerate(parents))
        for L in learners:
            L.close()


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
def test_brute_force(bnlib, spec):
    from bayesiannetwork_amd.learning import Learner
    crit = spec.criterion()
    _, table = BD.brute_input()
    bdt = BD.BDTable(table, spec)
    with info_table(table.pats, table.counts, table.k) as t:
        term = device_term(t, crit)
        # the hint enumeration (literal: a child reaches a parent node)
        with Learner(t, BD.BRUTE_HINT_START, crit, BD.MAX_PARENTS) as L:
            restated = BD.BDSearch(table.k, BD.BRUTE_HINT_START, bdt.term, BD.MAX_PARENTS)
            own = BD.BDSearch(table.k, BD.BRUTE_HINT_START, term, BD.MAX_PARENTS)
            score = L.brute_force_hint(*BD.BRUTE_HINT)
            restated.brute_force_hint(*BD.BRUTE_HINT)
            assert L.parents() == restated.parents and abs(score - restated.score) <= bdt.graph_bound(restated.parents)
            assert bits([score])[0] == bits([own.brute_force_hint(*BD.BRUTE_HINT)])[0] and L.parents() == own.parents
        # the full enumeration
        with Learner(t, None, crit, BD.MAX_PARENTS) as L:
            restated = BD.BDSearch(table.k, LR.empty_graph(5), bdt.term, BD.MAX_PARENTS)
            own = BD.BDSearch(table.k, LR.empty_graph(5), term, BD.MAX_PARENTS)
            ev, ev_own, ev_restated = L.brute_force(BD.BRUTE_VERTEXES), own.brute_force(BD.BRUTE_VERTEXES), restated.brute_force(BD.BRUTE_VERTEXES)
            assert bits([ev])[0] == bits([ev_own])[0] and L.parents() == own.parents and bits([L.score()])[0] == bits([own.score])[0]
            assert abs(ev - ev_restated) <= bdt.graph_bound(own.parents) + bdt.graph_bound(restated.parents)
            if spec.kind == 3:
                assert L.parents() == restated.parents
            assert sum(map(len, L.parents())) > 0


# ---- chains and runs, bit for bit over the device's own terms ----------------------------------------------------------

def table_term(rows, n):
    return lambda child, parents: float(rows[child][AR.rank(n, child, parents)])


def anneal_on_device(name, spec, chains=None, trace_chain=None):
    from bayesiannetwork_amd.learning import Learner, TermTable
    inp, q, rule, t0, t1, rate, boltz, same, cap, n_chains, seed = BD.ANNEAL[name]
    chains = n_chains if chains is None else chains
    crit = spec.criterion()
    _, table = AR.anneal_input(inp)
    with info_table(table.pats, table.counts, table.k) as t, TermTable(t, q, crit) as tt:
        rows = [tt.row(c) for c in range(table.n)]
        with Learner(t, BD.ANNEAL_START.get(name), crit) as L:
            rec = L.anneal(tt, t0, t1, rate, boltz, same, chains, seed, rule, cap, trace_chain=trace_chain)
            after = (L.score(), L.terms(), L.parents())
    pb = BD.BDProblem(table.k, q, table_term(rows, table.n), BD.ANNEAL_START.get(name))
    return rec, pb, AR.Schedule(t0, t1, rate, boltz, same, rule, cap), chains, seed, after


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
@pytest.mark.parametrize("name", list(BD.ANNEAL))
def test_chains_equal_the_restated_chain_bit_for_bit(bnlib, name, spec):
    trace_chain = 3 if BD.ANNEAL[name][9] < 100 else 129
    rec, pb, sched, chains, seed, after = anneal_on_device(name, spec, trace_chain=trace_chain)
    events = {}
    want = [AR.restated_chain(pb, sched, seed, j, events) for j in range(chains)]
    if name in BD.ANNEAL_START:   # the dense start: erases with a second round of 64, copies with a second trip
        assert all(events.get(key, 0) > 0 for key in ("erase_tail_gt64", "copy_gt64_accept", "copy_gt64_reject")), events
    for j, w in enumerate(want):
        assert AR.exp_margin_ok(w["uphill"]), f"chain {j}: an uphill decision within 2^-40 of its threshold: change the seed"
    for j, w in enumerate(want):
        assert bits([rec["eval"][j]])[0] == AR.bits(w["eval"]), j
        got = (int(rec["proposals"][j]), int(rec["operated"][j]), int(rec["accepted"][j]), int(rec["flags"][j]))
        assert got == (w["proposals"], w["operated"], w["accepted"], w["flags"]), j
        assert [int(x) for x in rec["masks"][j]] == w["masks"] and rec["edges"][j] == [tuple(e) for e in w["edges"]], j
    tr = [(int(x["method"]), int(x["from"]), int(x["to"]), int(x["now_bits"]), bool(x["accepted"])) for x in rec["trace"]]
    assert tr == want[trace_chain]["trace"] and len(tr) > 0
    evals = [w["eval"] for w in want]
    winner = evals.index(min(evals))                      # strictly smallest, the lowest index among equals
    score, (ll, params), parents = after
    assert rec["winner"] == winner and bits([score])[0] == AR.bits(want[winner]["eval"]) and score == BD.likelihood_alone(ll)
    assert np.array_equal(bits(ll), bits(want[winner]["ll"])) and parents == [list(AR._parents_of(m)) for m in want[winner]["masks"]]
    if name == "n33_met":                                  # a chain does not depend on the number of chains
        for fewer in (1, 5):
            part = anneal_on_device(name, spec, chains=fewer)[0]
            for key in ("eval", "proposals", "operated", "accepted", "flags", "masks"):
                assert np.array_equal(np.asarray(part[key]).view(np.uint8), np.asarray(rec[key][:fewer]).view(np.uint8)), (fewer, key)


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
def test_among_equal_evaluations_the_lowest_chain_wins(bnlib, spec):
    """Two proposals per chain on two nodes, seed 26: chains 2 and 3 end in the same, best graph -- evaluations with the same bits."""
    from bayesiannetwork_amd.learning import Learner, TermTable
    crit = spec.criterion()
    _, table = AR.anneal_input("n2")
    with info_table(table.pats, table.counts, table.k) as t, TermTable(t, 1, crit) as tt, Learner(t, None, crit) as L:
        rec = L.anneal(tt, 1.0, 1e-3, 0.5, chains=6, seed=26, rule="metropolis", max_proposals=2)
        best = rec["eval"].min()
        assert [j for j in range(6) if rec["eval"][j] == best] == [2, 3] and rec["winner"] == 2
        assert bits([L.score()])[0] == bits([best])[0] and L.parents() == [[1], []]


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
@pytest.mark.parametrize("name", list(BD.HC))
def test_hc_runs_equal_the_restated_run_bit_for_bit(bnlib, name, spec):
    from bayesiannetwork_amd.learning import Learner, TermTable
    inp, q, alpha, runs, seed = BD.HC[name]
    crit = spec.criterion()
    _, table = AR.anneal_input(inp)
    trace_run = min(runs - 1, 129)
    with info_table(table.pats, table.counts, table.k) as t, TermTable(t, q, crit) as tt:
        rows = [tt.row(c) for c in range(table.n)]
        kind = BD.HC_SIMILARITY.get(name)
        mi = HR.similarity_matrix(kind, table.n) if kind else t.pair_entropies()["mi"]
        given = {"similarity": mi} if kind else {}
        with Learner(t, None, crit) as L:
            rec = L.hc(tt, alpha, runs, seed, trace_run=trace_run, **given)
            score, (ll, _), parents = L.score(), L.terms(), L.parents()
            fewer = [(n_runs, L.hc(tt, alpha, n_runs, seed, **given)) for n_runs in (1, 5) if n_runs < runs]
    pb = BD.BDProblem(table.k, q, table_term(rows, table.n))
    events = {}
    want = [HR.restated_run(pb, mi, alpha, seed, j, events) for j in range(runs)]
    if kind == "nan_first":
        assert events.get("pick_nan_index0", 0) > 0 and events["p_nan"] == events["kept_pair"] > 0 and events.get("pick_tie_other_lane", 0) > 0
    elif kind == "inf_sparse":
        assert all(events.get(key, 0) > 0 for key in ("pick_tie_other_lane", "p_nan", "p_ge1", "p_zero", "pruned", "kept_pair")), events
    for j, w in enumerate(want):
        assert HR.pow_margin_ok(w["decisions"], alpha, w["exponents"]), f"run {j}: a pruning decision within 2^-40 of its threshold: change the seed"
    for j, w in enumerate(want):
        assert bits([rec["score"][j]])[0] == HR.bits(w["score"]), j
        got = tuple(int(rec[key][j]) for key in ("merges", "tried", "kept", "pruned", "pairs_kept", "flags"))
        assert got == (w["merges"], w["tried"], w["kept"], w["pruned"], w["pairs_kept"], w["flags"]), j
        assert [int(x) for x in rec["masks"][j]] == w["masks"], j
    w, cb = want[trace_run], HR.canonical_bits   # (a NaN's sign and payload are the machine's: hc_refs.canonical_bits)
    assert [(int(x.parent), int(x.child), cb(x.value_bits), int(x.coin)) for x in rec["merge_trace"]] == \
        [(p, c, cb(v), coin) for p, c, v, coin in w["merge_trace"]]
    assert [(int(x.cluster), int(x.connections), cb(x.value_bits), int(x.pruned)) for x in rec["prune_trace"]] == \
        [(c, k, cb(v), cut) for c, k, v, cut in w["prune_trace"]]
    scores = [w["score"] for w in want]
    winner = scores.index(min(scores))
    assert rec["winner"] == winner and bits([score])[0] == HR.bits(want[winner]["score"]) and score == BD.likelihood_alone(ll)
    assert parents == [list(AR._parents_of(m)) for m in want[winner]["masks"]]
    for n_runs, part in fewer:                             # a run does not depend on the number of runs
        assert np.array_equal(bits(part["score"]), bits(rec["score"][:n_runs])) and np.array_equal(part["masks"], rec["masks"][:n_runs])


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_name_the_cause_and_launch_nothing(bnlib):
    from bayesiannetwork_amd.evaluation import BDeu, K2Score
    from bayesiannetwork_amd.learning import Learner, TermTable, score_groups
    _, table = AR.anneal_input("n5")
    lib = _lib.lib()
    p32 = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    zero, ptr = np.zeros(1, np.int32), np.zeros(6, np.int32)
    out = np.zeros(4)
    f64 = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with info_table(table.pats, table.counts, table.k) as t:
        for ess in (0.0, -1.0, math.nan, math.inf, 2.0 ** -21, 2.0 ** 20 + 1.0):
            with pytest.raises(ValueError) as ei:
                BDeu(ess)
            assert "ess" in str(ei.value)
            spec = _lib.ScoreSpec(2, 0, ess)
            h = ctypes.c_void_p()
            calls = (lambda: lib.bn_learn_score_groups_spec(t._h, ctypes.byref(spec), 1, p32(zero), p32(np.zeros(2, np.int32)), None,
                                                            p32(np.zeros(2, np.int32)), None, f64, None),
                     lambda: lib.bn_learn_score_subsets_spec(t._h, ctypes.byref(spec), 0, 0, None, 0, None, f64, None),
                     lambda: lib.bn_learn_create_spec(t._h, p32(ptr), None, 2, ctypes.byref(spec), 4, ctypes.byref(h)),
                     lambda: lib.bn_terms_create_spec(t._h, ctypes.byref(spec), 2, ctypes.byref(h)))
            for call in calls:
                assert call() == _lib.BN_ERR_ARG and b"ess" in lib.bn_last_error() and not h.value, ess
        for ess in (2.0 ** -20, 2.0 ** 20):                                   # the ends of the range are taken
            assert len(score_groups(t, [(0, [], [])], criterion=BDeu(ess))) == 1
        for kind in (1, 4, -1):
            spec = _lib.ScoreSpec(kind, 0, 1.0)
            assert lib.bn_learn_score_groups_spec(t._h, ctypes.byref(spec), 1, p32(zero), p32(np.zeros(2, np.int32)), None,
                                                  p32(np.zeros(2, np.int32)), None, f64, None) == _lib.BN_ERR_ARG
            assert b"kind" in lib.bn_last_error()
        h = ctypes.c_void_p()
        k2 = _lib.ScoreSpec(3, 0, 0.0)
        assert lib.bn_learn_create_spec(t._h, p32(ptr), None, 2, ctypes.byref(k2), 4, ctypes.byref(h)) == _lib.BN_ERR_ARG and b"kind" in lib.bn_last_error()
        assert lib.bn_learn_create_spec(t._h, p32(ptr), None, 3, None, 4, ctypes.byref(h)) == _lib.BN_ERR_ARG and not h.value
        assert lib.bn_learn_create_spec(t._h, p32(ptr), None, 5, None, 4, ctypes.byref(h)) == _lib.BN_ERR_ARG and b"criterion" in lib.bn_last_error()
        assert lib.bn_learn_create(t._h, p32(ptr), None, 2, 4, ctypes.byref(h)) == _lib.BN_ERR_ARG                # the old entry point: 0 and 1 only
        with pytest.raises(ValueError):
            Learner(t, None, "bic")
        # a table / learner mismatch, both directions, through the library and through Python
        good = dict(initial_temp=10.0, final_temp=1.0, decreasing_rate=0.9)
        pairs = ((BDeu(1.0), "aic"), ("mdl", K2Score()), (BDeu(1.0), BDeu(2.0)), (BDeu(1.0), K2Score()), (K2Score(), BDeu(1.0)))
        for table_crit, learner_crit in pairs:
            with TermTable(t, 2, table_crit) as tt, Learner(t, None, learner_crit) as L:
                for run in (lambda: L.anneal(tt, **good), lambda: L.hc(tt, 0.5, 4)):
                    with pytest.raises(ValueError) as ei:
                        run()
                    assert "term table" in str(ei.value)
                p = _lib.AnnealParams(10.0, 1.0, 0.9, 1.0, 100, 1 << 20, 0, -1, 0, 0)
                w = ctypes.c_int32()
                assert lib.bn_learn_anneal(L._h, tt._h, ctypes.byref(p), 4, 0, None, None, None, None, None, None, ctypes.byref(w)) == _lib.BN_ERR_ARG
                assert b"term table" in lib.bn_last_error()
                hp = _lib.HcParams(0.5, 2, -1, 0, 0)
                assert lib.bn_learn_hc(L._h, tt._h, ctypes.byref(hp), 4, 0, None, None, None, None, None, None, ctypes.byref(w)) == _lib.BN_ERR_ARG
                assert b"term table" in lib.bn_last_error()
                assert L.info("anneal_chains") == 0 and L.info("hc_runs") == 0 and L.info("edges") == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------

def test_the_functors_return_the_score_evaluation_gives_bit_for_bit(bnlib):
    from bayesiannetwork_amd.evaluation import BDeu, K2Score
    from bayesiannetwork_amd.learning import K2, BruteForce, Greedy, Learner, SimulatedAnnealing, StepwiseStructure, StepwiseStructureHC, structure_model
    model, table = BD.learner_input()
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table.pats, table.counts, model.k) as t:
        sa = SimulatedAnnealing(BDeu(10), t, max_parents=2, chains=8, rule="metropolis", seed=5)
        hc = StepwiseStructureHC(K2Score(), t, max_parents=2, runs=8, seed=6)
        runs = ((Greedy("bdeu", t, max_parents=BD.MAX_PARENTS, seed=1), lambda f: f(start), BDeu()),
                (K2(K2Score, t, max_parents=BD.MAX_PARENTS, seed=2), lambda f: f(start), K2Score()),
                (sa, lambda f: f(start, 20.0, 0.5, 0.9), BDeu(10)),
                (hc, lambda f: f(start, 0.3), K2Score()),
                (StepwiseStructure(BDeu(2.0), t, inner=BruteForce, between=Greedy, seed=3, max_parents=3), lambda f: f(start, 3), BDeu(2.0)))
        for functor, call, ev in runs:
            learned, score = call(functor)
            learned.validate()
            assert learned.n_edges > 0 and bits([ev(learned, t)])[0] == bits([score])[0], type(functor).__name__
            with Learner(t, None, ev) as L0:
                assert score < L0.score()
        sa.close()
        hc.close()
