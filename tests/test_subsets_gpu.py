"""The subset lattice and the exhaustive searches on the GPU (bn_learn_score_subsets, bn_learn_best_parents, bn_learn_brute_force*,
bayesiannetwork_amd.learning.BruteForce / StepwiseStructure) against tests/subset_refs.py.

Counts are integers and compared exactly with direct counting; a family term of the lattice is compared BIT FOR BIT with
bn_learn_score_groups for the same family (ll is a function of the counts); the searches are compared bit for bit with the Python
restatement run over the device's own terms, and with the enumeration a user of the public API would write (fit_cpt -> Engine ->
AIC / MDL per enumerated graph) on the inputs whose margins tests/test_subsets_refs.py has checked: equal edges, score within B."""
import numpy as np
import pytest

import learning_refs as LR
import subset_refs as SR
from bayesiannetwork_amd import _lib
from pattern_refs import random_patterns

pytestmark = pytest.mark.gpu

# columns 0-16 binary; 17: k 3; 18: k 1; 19, 20: k 255; 21: k 17; 22: k 241; 23-27: k 16; 28: k 4; 29: k 5
KS = [2] * 17 + [3, 1, 255, 255, 17, 241] + [16] * 5 + [4, 5]
PATTERN_COUNTS = [1, 8, 2049]
CASES = [   # (child, base, candidates)
    (17, [], []), (17, [0, 28], []),                          # m = 0: the one family
    (17, [], [0]), (18, [17], [19]),                          # m = 1; a child of arity 1 with a candidate of arity 255
    (17, [5], [0, 18, 28, 9, 29]),                            # m = 5: candidates below, between and above the base id; arities 1, 4, 5
    (17, [9, 3], [28, 4, 1]),                                 # a base given in decreasing order
    (18, [], list(range(12))),                                # m = 12: top family of exactly 4 096 cells (the last one-launch size)
    (0, [], list(range(12, 0, -1))),                          # m = 12, 8 192 cells: one launch per level
    (16, list(range(8)), [10, 8, 9]),                         # eight base parents, 4 096 cells
    (17, list(range(8)), [8, 29, 28]),                        # eight base parents, 30 720 cells
    (25, [23], [24]), (21, [], [22]),                         # 4 096 and 4 097 cells: the boundary between the two forms
    (19, [], [20]), (25, [23], [0, 24]),                      # arities 255 and 16 beyond the boundary
    (27, [23, 24], [26, 25]),                                 # 2^20 cells: the cap
]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def weights(P, seed):
    r = np.random.default_rng(seed)
    return r.choice(np.array([1, 127, 128, (1 << 31) - 1, 1 << 31, 1 << 40], np.uint64), P)


def info_table(pats, counts, k):
    from bayesiannetwork_amd.evaluation import InfoTable
    return InfoTable(pats, counts, k, device=0)


def subset(cand, mask):
    return [cand[j] for j in range(len(cand)) if (mask >> j) & 1]


def device_terms(t):
    """ll_fn over bn_learn_score_groups, one family per call, cached."""
    from bayesiannetwork_amd.learning import score_groups
    cache = {}

    def ll(child, parents):
        key = (int(child), tuple(sorted(int(u) for u in parents)))
        if key not in cache:
            cache[key] = score_groups(t, [(key[0], list(key[1]), [])])[0][0]
        return cache[key]
    return ll


# ---- the lattice: exact counts, ll bit-equal to score_groups -------------------------------------------

@pytest.mark.parametrize("P", PATTERN_COUNTS)
def test_every_subset_has_the_counts_and_the_bits_of_score_groups(bnlib, P):
    from bayesiannetwork_amd.learning import score_groups, score_subsets
    pats, counts = random_patterns(KS, P, seed=P), weights(P, P + 1)
    rng = np.random.default_rng(P)
    with info_table(pats, counts, KS) as t:
        for child, base, cand in CASES:
            ll, N = score_subsets(t, child, base, cand, counts=True)
            assert len(ll) == len(N) == 1 << len(cand)
            assert np.array_equal(bits(score_subsets(t, child, base, cand)), bits(ll))   # (with and without the copy of the counts)
            for mask in range(1 << len(cand)):
                want = LR.family_counts(pats, counts, KS, child, base + subset(cand, mask))
                assert np.array_equal(N[mask], want), (child, base, cand, mask)
            # batched: every family as the base of a group of its own, one call
            groups = [(child, sorted(base + subset(cand, mask)), []) for mask in range(1 << len(cand))]
            batched = [x[0] for x in score_groups(t, groups)]
            assert np.array_equal(bits(batched), bits(ll)), (child, base, cand)
            # alone: one call per family (a sample of the large lattices), and as candidates of the base
            for mask in (range(1 << len(cand)) if len(cand) <= 5 else rng.choice(1 << len(cand), 24, replace=False)):
                alone = score_groups(t, [groups[int(mask)]])[0][0]
                assert bits([alone])[0] == bits([ll[int(mask)]])[0], (child, base, cand, mask)
            as_cand = score_groups(t, [(child, sorted(base), cand)])[0]
            assert np.array_equal(bits(as_cand), bits([ll[0]] + [ll[1 << j] for j in range(len(cand))]))


def test_no_result_depends_on_the_split_of_the_patterns(bnlib):
    from bayesiannetwork_amd.learning import score_subsets
    P = 2049
    pats, counts = random_patterns(KS, P, seed=5), weights(P, 6)
    with info_table(pats, counts, KS) as t:
        for child, base, cand in CASES:
            ll, N = score_subsets(t, child, base, cand, counts=True)
            for splits in (1, 2, 7):
                ll_s, N_s = score_subsets(t, child, base, cand, counts=True, splits=splits)
                assert np.array_equal(bits(ll_s), bits(ll)), (child, base, cand, splits)
                assert all(np.array_equal(a, b) for a, b in zip(N_s, N)), (child, base, cand, splits)


def test_limits_are_refused_with_a_message_naming_the_number(bnlib):
    from bayesiannetwork_amd.learning import Learner, score_subsets
    pats, counts = random_patterns(KS, 9, seed=1), np.ones(9, np.uint64)
    with info_table(pats, counts, KS) as t:
        def bad(args, text):
            with pytest.raises(_lib.BnError) as ei:
                score_subsets(t, *args)
            assert ei.value.code == _lib.BN_ERR_ARG and text in str(ei.value), str(ei.value)
        bad((17, list(range(9)), list(range(9, 17))), "17 parents")
        bad((27, [23, 24, 25], [26, 0]), "2^20 (1048576)")
        bad((16, [], list(range(16))), "at most 2^25 = 33554432")
        bad((17, [0], [1, 1]), "candidate 1 listed twice")
        bad((17, [0], [0]), "candidate 0 listed twice")
        bad((17, [0, 0], []), "parent 0 listed twice")
        bad((17, [0], [17]), "the child is among its candidates")
        bad((17, [30], []), "parent id 30")
        bad((17, [], [-1]), "candidate id -1")
        bad((30, [], []), "child id 30")
        with Learner(t, None, "aic") as L:
            with pytest.raises(_lib.BnError) as ei:   # sixteen survivors whose 2^16 tables pass the scratch: an error, not a cut
                L.best_parents(16, list(range(16)))
            assert "33554432" in str(ei.value) and L.info("edges") == 0
            with pytest.raises(_lib.BnError) as ei:
                L.brute_force(list(range(9)))
            assert "9 vertexes" in str(ei.value)
            with pytest.raises(_lib.BnError) as ei:
                L.brute_force([1, 2, 1])
            assert "twice" in str(ei.value)
            for call in (lambda: L.best_parents(30, [0]), lambda: L.best_parents(0, [30]), lambda: L.brute_force([30]),
                         lambda: L.brute_force_hint([30], [0]), lambda: L.brute_force_hint([0], [-1])):
                with pytest.raises(_lib.BnError):
                    call()
        with Learner(t, [[]] * 6 + [[0]] + [[]] * 23, "aic") as L:   # 0 -> 6: the child 0 reaches the parent node 6
            with pytest.raises(_lib.BnError) as ei:
                L.brute_force_hint([6, 7, 8], list(range(7)))
            assert "21 possible edges" in str(ei.value)


# ---- the searches against the restatement over the device's own terms: bit for bit ------------------------

def same(L, ref):
    ll, params = L.terms()
    return (L.parents() == ref.parents and bits([L.score()])[0] == bits([ref.score])[0] and np.array_equal(bits(ll), bits(ref.ll))
            and params == ref.params and L.info("parameters") == params)


@pytest.mark.parametrize("name", ["alarm2k_aic", "dag60_mdl"])
def test_the_searches_are_the_restatement_over_the_device_terms(bnlib, name):
    from bayesiannetwork_amd.learning import Learner
    model, table, criterion, max_parents, calls = SR.hint_calls(name)
    with info_table(table.pats, table.counts, model.k) as t:
        terms = device_terms(t)

        def pair(start, mp=max_parents):
            return Learner(t, start, criterion, mp), SR.RefSearch(model.k, start or LR.empty_graph(model.n), criterion, table.total, terms, mp)
        # best_parents: the child itself, a candidate twice, a parent, a node the child reaches; max_parents 2 cuts the subsets
        for mp in (max_parents, 2):
            L, ref = pair(None, mp)
            with L:
                assert same(L, ref)
                for par, (c,) in calls:
                    cand = [c] + par + par[:2]
                    assert L.best_parents(c, cand).tolist() == ref.best_parents(c, cand), (c, cand)
                    assert same(L, ref), c
                    assert L.best_parents(c, cand).tolist() == ref.best_parents(c, cand) and same(L, ref)   # (again: what is left)
                assert L.info("edges") > 0 and all(len(p) <= mp for p in L.parents())
                assert L.info("subsets_scored") > 0 and L.info("lattice_ns") > 0
        # learn_with_hint, decomposed: several children, parents in two orders, a child listed twice
        L, ref = pair(None)
        with L:
            done = 0
            for i in range(0, len(calls) - 2, 3):
                par = calls[i][0]
                children = [c for _, (c,) in calls[i:i + 3] if c not in par]
                if ref.decomposes(par, children):   # (else the literal enumeration: at most 15 possible edges)
                    done += 1
                    children = children + children[:1]
                got, want = L.brute_force_hint(par, children), ref.brute_force_hint(par, children)
                assert bits([got])[0] == bits([want])[0] and same(L, ref), (par, children)
            assert done >= 1
            # ... and with refusals: the graph learned so far, the roles swapped (parents and children overlap, cycles are refused)
            edges = [(u, c) for c, ps in enumerate(ref.parents) for u in ps][:3]
            assert len(edges) == 3
            par, children = sorted({c for _, c in edges}), sorted({u for u, _ in edges} | {edges[0][1]})
            assert not ref.decomposes(par, children)
            got, want = L.brute_force_hint(par, children), ref.brute_force_hint(par, children)
            assert bits([got])[0] == bits([want])[0] and same(L, ref)
        # operator(): from no edges, and from a graph with edges inside and into the set
        vs = SR.neighbourhood(model, calls, 5)
        for start, order in ((None, vs), (None, vs[::-1][:4]), ([[vs[1]] if v == vs[0] else [vs[4]] if v == vs[2] else [] for v in range(model.n)], vs)):
            L, ref = pair(start)
            with L:
                got, want = L.brute_force(order), ref.brute_force(order)
                assert bits([got])[0] == bits([want])[0] and same(L, ref), order
        L, ref = pair(None, 1)
        with L:
            assert bits([L.brute_force(vs)])[0] == bits([ref.brute_force(vs)])[0] and same(L, ref)
            assert all(len(p) <= 1 for p in L.parents())


# ---- against the loop over the public API ------------------------------------------------------------------

class PublicSearch(SR.RefSearch):
    """What a user of the parent library writes: per enumerated graph fit_cpt of the whole graph, an Engine, AIC / MDL."""

    def __init__(self, k, parents, criterion, t, table, max_parents):
        from bayesiannetwork_amd.evaluation import AIC, MDL
        super().__init__(k, parents, criterion, table.total, table.libm_ll, max_parents)
        self.t, self.table, self.ev, self.cache = t, table, (AIC if criterion == "aic" else MDL)(t), {}

    def _score(self, parents, vertexes=None):
        from bayesiannetwork_amd.engine import Engine, fit_cpt
        from bayesiannetwork_amd.learning import _csr, structure_model
        key = (tuple(tuple(sorted(p)) for p in parents), None if vertexes is None else tuple(vertexes))
        if key not in self.cache:
            m = structure_model(self.k, *_csr([sorted(p) for p in parents]))
            m.cpt[:] = fit_cpt(m, self.table.pats, self.table.counts, device=0)
            with Engine(m, device=0) as eng:
                self.cache[key] = self.ev(eng) if vertexes is None else self.ev(eng, list(vertexes))
        return self.cache[key]


@pytest.mark.parametrize("name", LR.INPUT_NAMES)
def test_hint_searches_take_the_decisions_of_the_public_api_enumeration(bnlib, name):
    from bayesiannetwork_amd.learning import Learner
    model, table, criterion, max_parents, calls = SR.hint_calls(name)
    with info_table(table.pats, table.counts, model.k) as t:
        pub = PublicSearch(model.k, LR.empty_graph(model.n), criterion, t, table, max_parents)
        with Learner(t, None, criterion, max_parents) as L:
            for par, child in calls:
                graph, score, _ = SR.literal_hint(pub, par, child)
                pub.parents = graph
                got = L.brute_force_hint(par, child)
                assert L.parents() == graph, (par, child)
                diff, B = abs(got - score), LR.graph_bound(table, graph, criterion)
                assert diff <= B, (par, child, diff, B)
            print(f"{name}: {len(pub.cache)} public evaluations, {L.info('edges')} edges, {L.info('subsets_scored')} subsets; "
                  f"last |score - public score| = {diff:.3g}, B = {B:.3g}")
            assert L.info("edges") > 0


@pytest.mark.parametrize("name,size", [("alarm2k_mdl", 5), ("dag60_mdl", 4), ("alarm2k_aic", 3)])
def test_brute_force_against_the_public_api_enumeration(bnlib, name, size):
    from bayesiannetwork_amd.learning import BruteForce, structure_model
    model, table, criterion, max_parents, calls = SR.hint_calls(name)
    vs = SR.neighbourhood(model, calls, size)
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table.pats, table.counts, model.k) as t:
        bf = BruteForce(criterion, t, max_parents=max_parents)
        learned, score = bf(start, vs)
        got = [learned.parents(v).tolist() for v in range(model.n)]
        pub = PublicSearch(model.k, LR.empty_graph(model.n), criterion, t, table, max_parents)
        _, _, leaves = SR.literal_brute_force(pub, vs)
        visited = {tuple(tuple(p) for p in g): s for g, s in leaves}
        assert tuple(tuple(p) for p in got) in visited                      # a graph the enumeration visits
        B = LR.graph_bound(table, got, criterion)
        mine = visited[tuple(tuple(p) for p in got)]
        assert abs(mine - bf.last_eval) <= B, (mine, bf.last_eval, B)        # its public-API score is the reported one, within B(G)
        assert abs(pub._score(got) - score) <= B                             # ... and so is the whole graph's
        for g, s in visited.items():                                         # no visited graph is better by more than the two bounds
            assert mine <= s + B + LR.graph_bound(table, [list(p) for p in g], criterion), g
        print(f"{name}: {len(visited)} graphs; edges {learned.n_edges}; |public - reported| = {abs(mine - bf.last_eval):.3g}, B = {B:.3g}")
        assert learned.n_edges > 0 and bf.last["subsets_scored"] == size * (1 << (size - 1))


# ---- stepwise_structure; Greedy / K2 after the refactor --------------------------------------------------------

def test_stepwise_structure_is_its_calls_on_one_learner(bnlib):
    from bayesiannetwork_amd.engine import fit_cpt
    from bayesiannetwork_amd.learning import BruteForce, Greedy, Learner, StepwiseStructure, structure_model
    model, table, criterion, _, max_parents = LR.learning_input("alarm2k_mdl")
    # brute force within and between the clusters: twelve columns, clusters of three, the small cluster always the parent
    k12 = [int(x) for x in model.k[:12]]
    start12 = structure_model(k12, np.zeros(13, np.int32), np.zeros(0, np.int32))
    with info_table(table.pats[:, :12], table.counts, k12) as t:
        clusters, pairs = [[4, 0, 9], [1, 11, 6], [7, 2, 10], [3, 8, 5]], [(1, 0), (0, 2), (0, 1)]
        sw = StepwiseStructure(criterion, t, inner=BruteForce, between=BruteForce, max_parents=max_parents)
        learned, score = sw(start12, 3, plan=(clusters, pairs))
        assert sw.last_plan == (clusters, pairs)
        with Learner(t, None, criterion, max_parents) as L:
            cl = [list(c) for c in clusters]
            for c in cl:
                L.brute_force(c)
            for p, c in pairs:
                L.brute_force_hint(cl[p], cl[c])
                cl = [x for i, x in enumerate(cl) if i not in (p, c)] + [cl[p] + cl[c]]
            assert len(cl) == 1 and sorted(cl[0]) == list(range(12))
            assert [learned.parents(v).tolist() for v in range(12)] == L.parents() and bits([score])[0] == bits([L.score()])[0]
            with Learner(t, None, criterion, max_parents) as L0:
                assert score < L0.score() and L.info("edges") > 0
        learned.validate()
        assert np.array_equal(learned.cpt, fit_cpt(learned, table.pats[:, :12], table.counts, device=0))
        assert sw.last["subsets_scored"] > 0 and sw.last["passes"] > 0
        one = StepwiseStructure(criterion, t, between=BruteForce, max_parents=max_parents)
        g3, _ = one(start12, 4, plan=([[0, 1, 2, 3]], []))              # one cluster from the start: nothing to merge
        assert one.last_plan == ([[0, 1, 2, 3]], []) and set(g3.in_idx.tolist()) <= {0, 1, 2, 3}
        with pytest.raises(ValueError):
            one(start12, 3, plan=(clusters, pairs[:2]))
    start = structure_model(model.k, model.in_ptr, model.in_idx)   # (its edges are cleared)
    with info_table(table.pats, table.counts, model.k) as t:
        # the default pairing, brute force inside and greedy between, from a fixed plan: the greedy's shuffles come from its seed
        order = [int(v) for v in np.random.default_rng(3).permutation(model.n)]
        clusters = [order[i::8] for i in range(8)]                   # 37 nodes: five clusters of 5, three of 4
        pairs = [(1, 0), (0, 5), (2, 3), (4, 0), (0, 1), (2, 1), (0, 1)]
        ga, sa = StepwiseStructure(criterion, t, between=Greedy(criterion, t, max_parents=max_parents, seed=5), max_parents=max_parents)(
            start, 5, plan=(clusters, pairs))
        with Learner(t, None, criterion, max_parents) as L:
            greedy, cl = Greedy(criterion, t, max_parents=max_parents, seed=5), [list(c) for c in clusters]
            for c in cl:
                L.brute_force(c)
            for p, c in pairs:
                greedy.hint_on(L, cl[p], cl[c])
                cl = [x for i, x in enumerate(cl) if i not in (p, c)] + [cl[p] + cl[c]]
            assert [ga.parents(v).tolist() for v in range(model.n)] == L.parents() and bits([sa])[0] == bits([L.score()])[0]
            assert L.info("edges") > 0
        # from a seed: reproducible, and the clusters are the reference's round-robin deal
        x, y = (StepwiseStructure(criterion, t, seed=11, max_parents=max_parents) for _ in range(2))
        (g1, s1), (g2, s2) = x(start, 4), y(start, 4)
        r1 = x.last_plan
        assert r1 == y.last_plan and np.array_equal(g1.in_idx, g2.in_idx) and np.array_equal(g1.in_ptr, g2.in_ptr) and s1 == s2
        assert len(r1[0]) == 10 and sorted(len(c) for c in r1[0]) == [3] * 3 + [4] * 7 and len(r1[1]) == 9
        assert sorted(v for c in r1[0] for v in c) == list(range(model.n)) and all(p != c for p, c in r1[1])
        g4, s4 = StepwiseStructure(criterion, t, seed=11, max_parents=max_parents)(start, 4, plan=r1)   # the recorded plan replays the run
        assert np.array_equal(g4.in_idx, g1.in_idx) and np.array_equal(g4.in_ptr, g1.in_ptr) and s4 == s1 and g1.n_edges > 0


def test_greedy_and_k2_are_unchanged_by_running_on_a_given_learner(bnlib):
    """The loops as they were written inside Greedy / K2 before they could run on a given learner, made by hand with the same
    generator: same edges, same score bits."""
    from bayesiannetwork_amd.learning import K2, Greedy, Learner, structure_model
    model, table, criterion, orders, max_parents = LR.learning_input("alarm2k_mdl")
    start = structure_model(model.k, np.zeros(model.n + 1, np.int32), np.zeros(0, np.int32))
    with info_table(table.pats, table.counts, model.k) as t:
        def by_hand(loop):
            with Learner(t, None, criterion, max_parents) as L:
                loop(L)
                return L.parents(), L.score()

        def check(result, want):
            learned, score = result
            assert [learned.parents(v).tolist() for v in range(model.n)] == want[0] and bits([score])[0] == bits([want[1]])[0]
            assert learned.n_edges > 0

        def greedy_loop(L, rng=None, vs=None):
            rng = rng or np.random.default_rng(7)
            vs = list(range(model.n)) if vs is None else list(vs)
            vs = [vs[i] for i in rng.permutation(len(vs))]
            for i in range(len(vs)):
                tail = vs[i + 1:]
                vs[i + 1:] = [tail[j] for j in rng.permutation(len(tail))]
                L.try_parents(vs[i], vs[i + 1:])

        def hint_loop(L):
            rng = np.random.default_rng(7)
            cs = list(range(20, model.n))
            cs = [cs[i] for i in rng.permutation(len(cs))]
            ps = list(range(20))
            for child in cs:
                ps = [ps[i] for i in rng.permutation(len(ps))]
                L.try_parents(child, ps)

        def k2_loop(L):
            pre = {v: list(x) for v, x in LR.K2_PRECONDITION.items()}
            for target in (int(v) for v in np.random.default_rng(7).permutation(model.n)):
                cand = [v for v in range(model.n) if v != target and v not in pre.get(target, ())]
                for u, ok in zip(cand, L.try_parents(target, cand)):
                    if ok:
                        pre.setdefault(u, []).append(target)

        check(Greedy(criterion, t, max_parents=max_parents, seed=7)(start), by_hand(greedy_loop))
        check(Greedy(criterion, t, max_parents=max_parents, seed=7)(start, list(range(5, 30))), by_hand(lambda L: greedy_loop(L, vs=range(5, 30))))
        check(Greedy(criterion, t, max_parents=max_parents, seed=7).learn_with_hint(start, list(range(20)), list(range(20, model.n))), by_hand(hint_loop))
        check(Greedy(criterion, t, max_parents=max_parents)(start, orders=orders), by_hand(lambda L: LR.run_greedy(L, orders)))
        check(K2(criterion, t, max_parents=max_parents, seed=7)(start, LR.K2_PRECONDITION), by_hand(k2_loop))
        g = Greedy(criterion, t, max_parents=max_parents, seed=7)     # two searches of one functor draw from one generator, as before
        g(start)
        rng = np.random.default_rng(7)
        by_hand(lambda L: greedy_loop(L, rng))
        check(g(start), by_hand(lambda L: greedy_loop(L, rng)))
