"""Structure learning on the GPU (bn_learn_* of include/bn_mi355x.h, bayesiannetwork_amd.learning) against tests/learning_refs.py.

Counts are integers and compared exactly; a family term is compared bit for bit with itself across groupings, positions and
splits (it is a function of the counts), and with libm through the stated bound (8u + gamma_{m+1}) * sum |t| (the device's
logarithm is taken to be within 2 ulp); decisions are compared with the loop a user of the existing public API would write
(fit_cpt -> Engine -> AIC / MDL per candidate) on inputs whose margins tests/test_learning_refs.py has checked to be more than
1000 x the bound at EVERY decision, so equality of the accepted edges is required without exception."""
import itertools
import math

import numpy as np
import pytest

import learning_refs as LR
from bayesiannetwork_amd import _lib
from pattern_refs import random_patterns

pytestmark = pytest.mark.gpu

# columns 0-16 binary; 17: k 3; 18: k 1; 19, 20: k 255; 21: k 17; 22: k 241; 23-27: k 16; 28: k 4; 29: k 5
KS = [2] * 17 + [3, 1, 255, 255, 17, 241] + [16] * 5 + [4, 5]
PATTERN_COUNTS = [1, 7, 8, 9, 2047, 2048, 2049, 4097]   # a lane's eight patterns, the 2048-pattern tile, two tiles and one more
GROUPS = [
    (17, [], []), (18, [], [17, 0]), (19, [], [20]),                       # no parent; arity 1; a 65 025-entry candidate (device memory)
    (17, [0], [18, 28]), (19, [18], []), (18, [17], [19]),                   # one parent; a parent of arity 1; a child of arity 1
    (17, [0, 28], [1]),                                                      # two parents
    (17, list(range(8)), [8, 29]),                                           # eight parents
    (16, list(range(16)), []),                                               # sixteen parents: 2^17 entries
    (25, [23, 24], [0]),                                                     # exactly 4 096 entries (the last LDS size); candidate: 8 192
    (21, [22], []),                                                          # 4 097: the first size counted in device memory
    (27, [23, 24, 25, 26], []),                                              # 2^20: the cap
    (17, [3, 9, 28], [u for u in range(30) if u not in (3, 9, 17, 28)]),     # candidates below, between and above the base ids; > 1 chunk
]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def weights(P, seed):
    r = np.random.default_rng(seed)
    return r.choice(np.array([1, 127, 128, (1 << 31) - 1, 1 << 31, 1 << 40], np.uint64), P)


def info_table(pats, counts, k):
    from bayesiannetwork_amd.evaluation import InfoTable
    return InfoTable(pats, counts, k, device=0)


def families_of(groups):
    for c, b, us in groups:
        yield c, list(b)
        for u in us:
            yield c, sorted(b + [u])


def flat(lists):
    return [x for row in lists for x in row]


# ---- contracts 1 and 3: exact counts in the fitted layout, ll against libm --------------------------

@pytest.mark.parametrize("P", PATTERN_COUNTS)
def test_counts_are_exact_and_ll_is_within_the_libm_bound(bnlib, P):
    from bayesiannetwork_amd.learning import score_groups
    pats, counts = random_patterns(KS, P, seed=P), weights(P, P + 1)
    with info_table(pats, counts, KS) as t:
        ll, N = score_groups(t, GROUPS, counts=True)
        worst = 0.0
        for (child, parents), got_ll, got_N in zip(families_of(GROUPS), flat(ll), flat(N)):
            want = LR.family_counts(pats, counts, KS, child, parents)
            assert np.array_equal(got_N, want), (child, parents)
            terms = LR.family_terms(want, KS[child])
            bound = LR.ll_bound(want, KS[child])
            err = abs(got_ll - math.fsum(terms.tolist()))
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (child, parents, err, bound)
        print(f"P = {P}: largest |ll - fsum| / bound over {len(flat(ll))} families: {worst:.3g}")


# ---- contract 2: ll is a function of the family's counts ---------------------------------------------

def test_ll_has_the_same_bits_alone_batched_permuted_and_for_every_split(bnlib):
    from bayesiannetwork_amd.learning import score_groups
    P = 4097
    pats, counts = random_patterns(KS, P, seed=3), weights(P, 4)
    with info_table(pats, counts, KS) as t:
        ll, N = score_groups(t, GROUPS, counts=True)
        by_family = {(c, tuple(p)): x for (c, p), x in zip(families_of(GROUPS), flat(ll))}
        for splits in (1, 2, 7):
            ll_s, N_s = score_groups(t, GROUPS, counts=True, splits=splits)
            assert np.array_equal(bits(flat(ll_s)), bits(flat(ll))), splits
            assert all(np.array_equal(a, b) for a, b in zip(flat(N_s), flat(N))), splits
        alone = [(c, p, []) for c, p in families_of(GROUPS)]                 # every family as the base of a group of its own
        for splits in (0, 1, 7):
            one_by_one = [score_groups(t, [g], splits=splits)[0][0] for g in alone]
            assert np.array_equal(bits(one_by_one), bits(flat(ll))), splits
        assert np.array_equal(bits(flat(score_groups(t, alone))), bits(flat(ll)))
        permuted = [(c, b, list(reversed(us))) for c, b, us in reversed(GROUPS)]
        ll_p = score_groups(t, permuted)
        for (c, p), x in zip(families_of(permuted), flat(ll_p)):
            assert bits([x])[0] == bits([by_family[(c, tuple(p))]])[0], (c, p)
        # a family as a candidate of a different base: {3, 9, 28} + 5 reached from the bases {3, 9, 28}, {5, 9, 28}, {3, 5, 9}
        want = by_family[(17, (3, 5, 9, 28))]
        for base, u in (([5, 9, 28], 3), ([3, 5, 9], 28), ([3, 5, 28], 9)):
            assert bits([score_groups(t, [(17, base, [0, u])])[0][2]])[0] == bits([want])[0]
        # a batch whose count scratch passes 256 MiB runs in several passes: 34 families of 2^20 cells, with small ones between
        big, small = (27, [23, 24, 25, 26], []), (17, [0], [18, 28])
        many = flat(score_groups(t, [big, small] * 34))
        assert np.array_equal(bits(many), bits(([by_family[(27, (23, 24, 25, 26))]] + [by_family[(17, p)] for p in ((0,), (0, 18), (0, 28))]) * 34))
    # the same samples as other rows: shuffled, and every row split in two rows of half the weight
    order = np.random.default_rng(5).permutation(P)
    with info_table(pats[order], counts[order], KS) as t:
        assert np.array_equal(bits(flat(score_groups(t, GROUPS))), bits(flat(ll)))
    half = counts // np.uint64(2)
    with info_table(np.concatenate([pats, pats]), np.concatenate([half, counts - half]), KS) as t:
        assert np.array_equal(bits(flat(score_groups(t, GROUPS))), bits(flat(ll)))


# ---- the base family against the existing scores -----------------------------------------------------

def test_base_terms_agree_with_log_likelihood_nodes_of_the_fitted_engine(bnlib):
    """bn_score_nodes takes libm's logarithm of the same theta and adds in the same order: per node both lie within
    gamma_{m+1} * sum |t| of the exact sum of their own terms, and the terms differ by < 8u each: 8u + 2 gamma_{m+1} per node.
    The whole score: contract 4's B(G)."""
    from bayesiannetwork_amd.engine import Engine, fit_cpt
    from bayesiannetwork_amd.evaluation import AIC, MDL, log_likelihood_nodes
    from bayesiannetwork_amd.learning import Learner, score_groups, structure_model
    model, table, _, _, _ = LR.learning_input("alarm2k_mdl")
    with info_table(table.pats, table.counts, model.k) as t:
        ll = flat(score_groups(t, [(v, model.parents(v).tolist(), []) for v in range(model.n)]))
        fitted = structure_model(model.k, model.in_ptr, model.in_idx)
        fitted.cpt[:] = fit_cpt(fitted, table.pats, table.counts, device=0)
        parents = [model.parents(v).tolist() for v in range(model.n)]
        with Engine(fitted, device=0) as eng:
            pub = log_likelihood_nodes(eng, t)
            for v in range(model.n):
                _, mag, m = table.family(v, parents[v])
                assert pub[v] == table.libm_ll(v, parents[v])                 # (the restatement IS the public API)
                assert abs(ll[v] - pub[v]) <= (8 * LR.U + 2 * LR.gamma(m + 1)) * mag, v
            for criterion, ev in (("aic", AIC(t)), ("mdl", MDL(t))):
                with Learner(t, model, criterion) as L:
                    diff, B = abs(L.score() - ev(eng)), LR.graph_bound(table, parents, criterion)
                    print(f"{criterion}: |learner score - public score| = {diff:.3g}, B = {B:.3g}")
                    assert diff <= B
                    assert L.score() == LR.score_arith(ll, L.info("parameters"), criterion, table.total)
                    assert L.parents() == parents and L.info("edges") == model.n_edges


# ---- contract 6: the scan is the sequential loop -------------------------------------------------------

def device_ll(t):
    from bayesiannetwork_amd.learning import score_groups
    cache = {}

    def ll(child, parents):
        key = (child, tuple(parents))
        if key not in cache:
            cache[key] = score_groups(t, [(child, list(parents), [])])[0][0]
        return cache[key]
    return ll


@pytest.mark.parametrize("name", LR.INPUT_NAMES)
def test_the_scan_is_the_sequential_loop_over_the_device_terms(bnlib, name):
    from bayesiannetwork_amd.learning import Learner
    model, table, criterion, orders, max_parents = LR.learning_input(name)
    with info_table(table.pats, table.counts, model.k) as t:
        ref = LR.RefLearner(model.k, LR.empty_graph(model.n), criterion, table.total, device_ll(t), max_parents)
        with Learner(t, None, criterion, max_parents) as L:
            assert bits([L.score()])[0] == bits([ref.score])[0]
            passes = 1
            for child, tail in zip(*orders):
                want = ref.try_parents(child, tail)
                got = L.try_parents(child, tail)
                assert got.tolist() == want, child
                assert bits([L.score()])[0] == bits([ref.score])[0], child
                passes += sum(want) + 1
            assert L.parents() == ref.parents
            assert L.info("passes") <= passes and L.info("families_scored") >= model.n


# ---- contract 5: decisions against the loop over the existing public API -------------------------------

class PublicLoop:
    """What a user of the parent library writes: per candidate edge fit_cpt of the whole graph, an Engine, AIC / MDL."""

    def __init__(self, k, parents, criterion, t, table, max_parents):
        from bayesiannetwork_amd.evaluation import AIC, MDL
        self.k, self.n, self.t, self.table, self.max_parents = [int(x) for x in k], len(k), t, table, max_parents
        self.ev = (AIC if criterion == "aic" else MDL)(t)
        self.parents = [sorted(p) for p in parents]
        self.score = self.evaluate(self.parents)
        self.evaluations = 0

    def evaluate(self, parents):
        from bayesiannetwork_amd.engine import Engine, fit_cpt
        from bayesiannetwork_amd.learning import _csr, structure_model
        m = structure_model(self.k, *_csr(parents))
        m.cpt[:] = fit_cpt(m, self.table.pats, self.table.counts, device=0)
        with Engine(m, device=0) as eng:
            return self.ev(eng)

    def try_parents(self, child, cand):
        out = []
        for u in cand:
            par = self.parents[child]
            if u == child or u in par or u in LR.reaches(self.parents, child) or len(par) + 1 > self.max_parents:
                out.append(False)
                continue
            nxt = [list(p) for p in self.parents]
            nxt[child] = sorted(par + [u])
            score_next = self.evaluate(nxt)
            self.evaluations += 1
            take = score_next < self.score
            if take:
                self.parents, self.score = nxt, score_next
            out.append(take)
        return out


def check_against_public_loop(name, kind):
    from bayesiannetwork_amd.learning import Learner
    model, table, criterion, orders, max_parents = LR.learning_input(name)
    with info_table(table.pats, table.counts, model.k) as t:
        pub = PublicLoop(model.k, LR.empty_graph(model.n), criterion, t, table, max_parents)
        with Learner(t, None, criterion, max_parents) as L:
            if kind == "greedy":
                want, got = LR.run_greedy(pub, orders), LR.run_greedy(L, orders)
                assert [list(x) for x in got] == want
            elif kind == "hint":
                o = LR.hint_orders(model.n, 31)
                assert [list(x) for x in LR.run_hint(L, o)] == LR.run_hint(pub, o)
            else:
                ch = LR.k2_children(model.n, 41)
                want, got = LR.run_k2(pub, ch, LR.K2_PRECONDITION), LR.run_k2(L, ch, LR.K2_PRECONDITION)
                assert [(c, [bool(x) for x in f]) for c, f in got] == want
            assert L.parents() == pub.parents and L.info("edges") > 0
            diff, B = abs(L.score() - pub.score), LR.graph_bound(table, pub.parents, criterion)
            print(f"{name} {kind}: {pub.evaluations} decisions, {L.info('edges')} edges, {L.info('passes')} passes, "
                  f"{L.info('families_scored')} families; |score - public score| = {diff:.3g}, B = {B:.3g}")
            assert diff <= B


@pytest.mark.parametrize("name", LR.INPUT_NAMES)
def test_greedy_takes_the_decisions_of_the_public_api_loop(bnlib, name):
    check_against_public_loop(name, "greedy")


@pytest.mark.parametrize("kind", ["hint", "k2"])
def test_hint_and_k2_take_the_decisions_of_the_public_api_loop(bnlib, kind):
    check_against_public_loop("alarm2k_mdl", kind)


# ---- the Python functors, a starting graph, max_parents, the error paths --------------------------------

def test_greedy_and_k2_functors_return_the_fitted_model_and_the_learners_score(bnlib):
    from bayesiannetwork_amd.engine import Sampler, fit_cpt
    from bayesiannetwork_amd.learning import K2, Greedy, Learner, structure_model
    model, table, criterion, orders, max_parents = LR.learning_input("alarm2k_mdl")
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table.pats, table.counts, model.k) as t:
        with Learner(t, None, criterion, max_parents) as L:
            LR.run_greedy(L, orders)
            want_parents, want_score = L.parents(), L.score()
        g = Greedy("mdl", t, max_parents=max_parents)
        learned, score = g(start, orders=orders)
        assert [learned.parents(v).tolist() for v in range(model.n)] == want_parents and score == want_score
        learned.validate()
        assert np.array_equal(learned.cpt, fit_cpt(learned, table.pats, table.counts, device=0))
        assert g.last["passes"] > 0 and g.last["families_scored"] > model.n
        # shuffles from a seed: reproducible, a DAG, and a score below the empty graph's
        a, sa = Greedy("mdl", t, max_parents=max_parents, seed=7)(start)
        b, sb = Greedy("mdl", t, max_parents=max_parents, seed=7)(start)
        assert np.array_equal(a.in_idx, b.in_idx) and sa == sb
        with Learner(t, None, "mdl") as L0, Learner(t, a, "mdl") as La:    # (the learned graph as a STARTING graph: acyclic, same score)
            assert sa < L0.score() and La.score() == sa
        sub = list(range(10, 30))
        c, _ = Greedy("aic", t, seed=1)(start, sub)
        assert all(set(c.parents(v).tolist()) <= set(sub) for v in sub) and all(len(c.parents(v)) == 0 for v in range(10))
        h, _ = Greedy("mdl", t, seed=2).learn_with_hint(start, list(range(20)), list(range(20, model.n)))
        assert all(len(h.parents(v)) == 0 for v in range(20)) and all(u < 20 for u in h.in_idx.tolist())
        k2, s2 = K2("mdl", t, max_parents=max_parents)(start, LR.K2_PRECONDITION, orders=LR.k2_children(model.n, 41))
        with Learner(t, None, "mdl", max_parents) as L:
            LR.run_k2(L, LR.k2_children(model.n, 41), LR.K2_PRECONDITION)
            assert [k2.parents(v).tolist() for v in range(model.n)] == L.parents() and s2 == L.score()
        assert not set(k2.parents(36).tolist()) & set(range(20))
    # a Sampler as the sampling: marshalled over every node in node order
    smp = Sampler()
    smp.load_sample({tuple(int(x) for x in row): int(c) for row, c in zip(table.pats, table.counts)})
    learned2, score2 = Greedy("mdl", smp, max_parents=max_parents)(start, orders=orders)
    assert np.array_equal(learned2.in_idx, learned.in_idx) and score2 == score


def test_a_starting_graph_with_edges_max_parents_and_refused_candidates(bnlib):
    from bayesiannetwork_amd.learning import Learner
    k = [2] * 8
    pats = np.zeros((256, 8), np.uint8)
    pats[:, :6] = np.tile(np.array(list(itertools.product([0, 1], repeat=6)), np.uint8), (4, 1))   # every combination, four times
    pats[:, 7] = pats[:, 0] ^ pats[:, 1] ^ pats[:, 2] ^ pats[:, 3]           # only all four together explain column 7 ...
    pats[:, 6] = pats[:, 5]                                                   # ... and 6 copies 5
    counts = np.full(256, 40, np.uint64)
    table = LR.Table(pats, counts, k)
    with info_table(pats, counts, k) as t:
        start = [[], [], [], [], [], [], [], [1, 0, 2]]                       # (any parent order is taken)
        for max_parents, expect in ((4, [0, 1, 2, 3]), (3, [0, 1, 2])):
            with Learner(t, start, "aic", max_parents) as L:
                ref = LR.RefLearner(k, start, "aic", table.total, device_ll(t), max_parents)
                cand = [7, 0, 4, 3, 3, 5]                                      # the child; a parent; no gain; the gain (if allowed); twice
                assert L.try_parents(7, cand).tolist() == ref.try_parents(7, cand)
                assert L.parents()[7] == expect == ref.parents[7] and L.score() == ref.score
        with Learner(t, [[], [0], [1], [], [], [], [5], []], "mdl") as L:     # 0 -> 1 -> 2, 5 -> 6
            assert L.try_parents(0, [2, 1]).tolist() == [False, False]         # both would close a cycle
            assert L.try_parents(5, [6]).tolist() == [False] and L.info("passes") == 1   # (no device pass for nothing to score)
            assert L.try_parents(6, [5, 0]).tolist() == [False, False] and L.parents()[6] == [5]
            assert L.try_parents(3, []).tolist() == []
        with Learner(t, None, "mdl", 0) as L:
            assert L.try_parents(6, [5]).tolist() == [False]


def test_error_paths_name_the_group(bnlib):
    from bayesiannetwork_amd.learning import Learner, score_groups
    pats, counts = random_patterns(KS, 9, seed=1), np.ones(9, np.uint64)
    with info_table(pats, counts, KS) as t:
        def bad(groups, text):
            with pytest.raises(_lib.BnError) as ei:
                score_groups(t, groups)
            assert ei.value.code == _lib.BN_ERR_ARG and text in str(ei.value), str(ei.value)
        ok = (17, [0], [1])
        bad([ok, (30, [], [])], "group 1: child id 30")
        bad([(17, [1, 0], [])], "group 0: base parents must be strictly increasing")
        bad([ok, ok, (17, [0, 17], [])], "group 2: the child is among its parents")
        bad([(17, [0], [0])], "group 0: candidate 0 is already a base parent")
        bad([(17, [0], [1, 1])], "group 0: candidate 1 listed twice")
        bad([(17, [0], [17])], "group 0: the child is among its candidates")
        bad([(17, [0], [-1])], "group 0: candidate id -1")
        bad([ok, (16, list(range(16)), [17])], "group 1: a family of 17 parents")
        bad([(17, list(range(17)), [])], "group 0: a family of 17 parents")
        bad([(27, [23, 24, 25, 26], [0])], "group 0: a family table of more than 2^20 entries")
        bad([(19, [20, 21, 22], [])], "group 0: a family table of more than 2^20 entries")
        assert score_groups(t, []) == []
        for structure, text in (([[1], [0]] + [[]] * 28, "cycle"), ([[1, 1]] + [[]] * 29, "twice"), ([[0]] + [[]] * 29, "itself"),
                                ([[]] * 17 + [list(range(17))] + [[]] * 12, "17 parents")):
            with pytest.raises(_lib.BnError) as ei:
                Learner(t, structure, "aic")
            assert ei.value.code == _lib.BN_ERR_ARG and text in str(ei.value), str(ei.value)
        with pytest.raises(_lib.BnError):
            Learner(t, None, "aic", 17)
        with Learner(t, None, "aic") as L:
            for args in ((30, [0]), (0, [30]), (-1, [])):
                with pytest.raises(_lib.BnError) as ei:
                    L.try_parents(*args)
                assert ei.value.code == _lib.BN_ERR_ARG
            with pytest.raises(_lib.BnError):
                L.info("nothing")
            # the over-limit candidate is skipped, not an error: 27 <- 23, 24, 25, 26 is at the cap
        with Learner(t, [[]] * 27 + [[23, 24, 25, 26]] + [[]] * 2, "aic") as L:
            assert L.try_parents(27, [0, 28]).tolist() == [False, False] and L.info("passes") == 1


# ---- a batch whose passes cut THROUGH its groups ----------------------------------------------------

def _passes_of(ks, groups):
    """The pass of every family of a batch, family by family in input order, by the rule bn_learn.hpp states: a family of at most
    4 096 cells is counted in LDS (chunks of <= 32 candidates and <= 4 096 cells), the others in device memory (chunks of <= 8
    candidates); a group's LDS chunks come first; a pass is a run of whole chunks of at most 2^25 cells."""
    chunks = []                                                              # (cells, [family indices])
    fam = 0
    for c, b, us in groups:
        base = ks[c] * math.prod(ks[x] for x in b)
        cells = [base] + [base * ks[u] for u in us]
        for lds in (True, False):
            cur = None
            for j, x in enumerate(cells):
                if (x <= 4096) != lds:
                    continue
                n_cand = sum(1 for f in cur[1] if f != fam) if cur else 0
                if cur is None or n_cand >= (32 if lds else 8) or (lds and cur[0] + x > 4096):
                    cur = [0, []]
                    chunks.append(cur)
                cur[0] += x
                cur[1].append(fam + j)
        fam += len(cells)
    passes, at, p = [0] * fam, 0, 0
    for cells, fams in chunks:
        if at > 0 and at + cells > (1 << 25):
            p, at = p + 1, 0
        at += cells
        for f in fams:
            passes[f] = p
    return passes


def test_a_group_scored_by_more_than_one_pass_has_the_bits_of_its_families_scored_alone(bnlib):
    """200 patterns over 120 variables: 0-9 of arity 4 (1-9 mostly in state 0, so that rows hold several patterns), 10-49 of
    arity 1, 50-83 of arity 255 (three states in use), 84-119 of arity 4.  One call scores three groups of child 0:
    A: base 1..9 (4^10 = 2^20 cells, exactly the per-family limit) and the 40 candidates of arity 1: 41 families of 2^20 cells in
       device-memory chunks of 9, 8, 8, 8, 8 families; the 2^25-cell scratch ends the first pass after A's third chunk.
    B: base 1..5 (4 096 cells, the last LDS size), candidates alternately of arity 1 (LDS chunks, which come first) and of arity
       255 (1 044 480 cells, device memory): a pass ends inside B's device-memory chunks, so B's families do NOT go to the passes
       in input order and their scores come back through the reorder.
    C: base 1..8 (2^18 cells) and 37 candidates of arity 4 (2^20 cells each, every one another function of the data).
    Five passes; each group has families in two of them.  Expected: every family as a group of its own, one pass each."""
    from bayesiannetwork_amd.learning import score_groups
    ks = [4] * 10 + [1] * 40 + [255] * 34 + [4] * 36
    A = (0, list(range(1, 10)), list(range(10, 50)))
    B = (0, list(range(1, 6)), flat([[10 + j, 50 + j] for j in range(34)]))
    C = (0, list(range(1, 9)), [9] + list(range(84, 120)))
    groups = [A, B, C]
    passes = _passes_of(ks, groups)
    pa, pb, pc = passes[:41], passes[41:110], passes[110:]
    assert len(pc) == 38 and max(passes) + 1 >= 2 and all(len(set(p)) >= 2 for p in (pa, pb, pc))
    assert pa == sorted(pa) and pb != sorted(pb)                             # A goes in input order; B is reordered
    alone = [(c, p, []) for c, p in families_of(groups)]
    assert all(max(_passes_of(ks, [g])) == 0 for g in alone)
    r = np.random.default_rng(41)
    pats = random_patterns(ks, 200, seed=42)
    pats[:, 1:10] *= (r.random((200, 9)) < 0.2).astype(np.uint8)
    pats[:, 50:84] = 100 * r.integers(0, 3, (200, 34)).astype(np.uint8)
    with info_table(pats, weights(200, 43), ks) as t:
        got = score_groups(t, groups)
        want = [score_groups(t, [g])[0][0] for g in alone]
        assert [len(x) for x in got] == [41, 69, 38]
        assert np.array_equal(bits(flat(got)), bits(want))
        assert len(set(bits(want).tolist())) >= 60                           # (a misplaced score would show: the families differ)
