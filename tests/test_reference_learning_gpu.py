"""The device's CPT fitting, scores and structure searches against the REFERENCE'S OWN CODE: tests/golden/learn_*.npz hold what
the unmodified sampler.hpp, aic / mdl, greedy, k2_algorithm, brute_force and stepwise_structure did on the project's fixed inputs
(tests/reference_learning.py; tests/test_reference_learning_golden.py checks the fixtures themselves and the margin condition on
the CPU).  Reads nothing but tests/golden/.  Largest input: 37 nodes, 3 000 patterns.

Exact ties.  brute_force -- alone and as stepwise_structure's inner learning -- compares graphs whose AIC / MDL are EQUAL in exact
arithmetic (a -> b against b -> a); which of the two wins is settled by the rounding of whoever adds the terms.  Where the device
may end in such a twin the tests accept exactly that and nothing else: the reference's graph, or one that RL.exact_tie proves
equal to it in integer arithmetic; every decision that exact arithmetic does decide is demanded as the reference took it."""
import numpy as np
import pytest

import learning_refs as LR
import reference_learning as RL

pytestmark = pytest.mark.gpu


def ids(pairs):
    return [f"{name}-{i}-{RL.load(name)[1][i]!r}" for name, i in pairs]


def cases(kinds):
    pairs = RL.all_runs(kinds)
    return pytest.mark.parametrize("name,index", pairs, ids=ids(pairs))


@pytest.fixture(scope="module")
def tables(bnlib):
    """One device table per fixture, uploaded once for the module."""
    from bayesiannetwork_amd.evaluation import InfoTable
    opened = {}

    def get(name):
        if name not in opened:
            table, _ = RL.load(name)
            opened[name] = InfoTable(table.pats, table.counts, table.k, device=0)
        return opened[name]
    yield get
    for t in opened.values():
        t.close()


def fitted_model(table, parents):
    from bayesiannetwork_amd.engine import fit_cpt
    from bayesiannetwork_amd.learning import structure_model
    ptr, idx = RL._ragged(parents, np.int32)
    model = structure_model(table.k, ptr, idx)
    model.cpt[:] = fit_cpt(model, table.pats, table.counts, device=0)
    return model


def same_or_tied(table, got, run, vertexes=None):
    return got == run.final or RL.exact_tie(table, got, run.final, vertexes)


def value_bound(table, got, run, vertexes=None):
    """The device's value for `got` against the reference's for run.final: one bound for the same graph, the two graphs' bounds for
    an exactly tied twin (both values approximate the same exact number)."""
    B = LR.reference_bound(table, run.final, run.criterion, vertexes)
    return B if got == run.final else B + LR.reference_bound(table, got, run.criterion, vertexes)


# ---- CPTs ---------------------------------------------------------------------------------------------------------------

@cases(("make_cpt",))
def test_fit_cpt_has_the_references_bits(bnlib, name, index):
    table, runs = RL.load(name)
    run = runs[index]
    got = fitted_model(table, run.start).cpt
    assert got.shape == run.cpt.shape and np.array_equal(got.view(np.uint64), run.cpt.view(np.uint64))


def test_fit_cpt_gives_the_uniform_row_where_the_reference_does(bnlib):
    rows = 0
    for name, index in RL.all_runs(("make_cpt",)):
        table, runs = RL.load(name)
        model = fitted_model(table, runs[index].start)
        for v in range(table.n):
            kv = int(table.k[v])
            N = LR.family_counts(table.pats, table.counts, table.k, v, runs[index].start[v]).reshape(-1, kv)
            for r in np.nonzero(N.sum(axis=1) == 0)[0]:
                o = int(model.cpt_off[v]) + int(r) * kv
                assert np.all(model.cpt[o:o + kv] == 1.0 / kv) and np.array_equal(model.cpt[o:o + kv], runs[index].cpt[o:o + kv])
                rows += 1
    assert rows >= 10


# ---- scores of fitted models ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RL.fixture_names())
def test_scores_of_fitted_models_agree_with_the_reference(bnlib, tables, name):
    """AIC / MDL of the engine with fitted CPTs against the reference's double, for every score run (both forms) and for the
    final graph of every search (whose return value is the reference's score of it)."""
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import AIC, MDL
    table, runs = RL.load(name)
    t = tables(name)
    checked, worst = 0, 0.0
    for run in runs:
        if run.kind == "make_cpt":
            continue
        if run.kind == "score":
            parents, vs = run.start, run.vertexes
        else:
            parents = run.final
            vs = run.vertexes if run.kind == "brute_vertexes" else list(range(table.n)) if run.kind == "brute_all" else None
        ev = (AIC if run.criterion == "aic" else MDL)(t)
        with Engine(fitted_model(table, parents), device=0) as eng:
            got = ev(eng) if vs is None else ev(eng, vs)
            B = LR.reference_bound(table, parents, run.criterion, vs)
            print(f"{name} {run!r}: |device - reference| = {abs(got - run.value):.3g}, bound {B:.3g}")
            assert abs(got - run.value) <= B, (run, got, run.value, B)
            worst = max(worst, abs(got - run.value) / B)
            if vs is not None:   # the vertex-list form is calc_likelihood over those nodes plus the WHOLE graph's penalty
                params = sum(LR.family_params(table.k, v, ps) for v, ps in enumerate(parents))
                alone = ev.calc_likelihood(eng, vs) + float(params) * LR.penalty_factor(run.criterion, table.total)
                assert abs(alone - run.value) <= B
            checked += 1
    print(f"{name}: {checked} graphs, largest |difference| / bound {worst:.3g}")
    assert checked > 0


# ---- greedy, greedy with hint, K2 ---------------------------------------------------------------------------------------------------

@cases(RL.TRY_KINDS)
def test_the_learner_takes_the_references_decisions(bnlib, tables, name, index):
    from bayesiannetwork_amd.learning import K2, Greedy, Learner
    table, runs = RL.load(name)
    run, t = runs[index], tables(name)
    decisions = RL.try_segment(table.n, run.evals, 0, len(run.evals), RL.edge_set(run.final))
    children, tails = RL.orders_of(decisions)
    want = [kept for *_, kept, _ in decisions]
    B = LR.reference_bound(table, run.final, run.criterion)
    with Learner(t, run.start, run.criterion) as L:   # the log's visits, one try_parents per visited child
        got = [bool(f) for child, tail in zip(children, tails) for f in L.try_parents(child, tail)]
        assert got == want and L.parents() == run.final
        assert abs(L.score() - run.value) <= B, (L.score(), run.value, B)
    with Learner(t, run.start, run.criterion) as L:   # the same through the search classes, the shuffles replaced by the log's orders
        if run.kind == "k2":
            order = children + [v for v in range(table.n) if v not in children]
            score = K2(run.criterion, t).run_on(L, run.precondition, orders=order)
        elif run.kind == "greedy_hint":
            score = Greedy(run.criterion, t).hint_on(L, run.hint[0], run.hint[1], orders=(children, tails))
        else:
            score = Greedy(run.criterion, t).run_on(L, run.vertexes, orders=(children, tails))
        assert L.parents() == run.final and score == L.score()
        assert abs(score - run.value) <= B


# ---- brute force ------------------------------------------------------------------------------------------------------------------

@cases(RL.BRUTE_KINDS)
def test_brute_force_ends_in_the_references_best_graph(bnlib, tables, name, index):
    from bayesiannetwork_amd.learning import BruteForce, Learner
    table, runs = RL.load(name)
    run, t = runs[index], tables(name)
    with Learner(t, run.start, run.criterion) as L, Learner(t, run.start, run.criterion) as L2:
        bf = BruteForce(run.criterion, t)
        if run.kind == "brute_hint":
            vs = None
            got = L.brute_force_hint(*run.hint)
            assert bf.hint_on(L2, *run.hint) == got
        else:
            vs = list(range(table.n)) if run.kind == "brute_all" else run.vertexes
            got = L.brute_force(vs)
            bf.run_on(L2, vs)
            assert bf.last_eval == got
        assert same_or_tied(table, L.parents(), run, vs), (L.parents(), run.final)
        assert L2.parents() == L.parents()
        B = value_bound(table, L.parents(), run, vs)
        print(f"{name} {run!r}: same graph {L.parents() == run.final}; |device - reference| = {abs(got - run.value):.3g}, bound {B:.3g}")
        assert abs(got - run.value) <= B, (got, run.value, B)


# ---- stepwise_structure ---------------------------------------------------------------------------------------------------------------

@cases(("stepwise",))
def test_stepwise_structure_follows_the_references_plan(bnlib, tables, name, index):
    """The plan (clusters, merges) and the between-learning orders all come from the reference's own calls and log.  Twice: (1)
    StepwiseStructure end to end, `between` an instance that hands hint_on the log's orders per merge; (2) the between phase alone
    on a learner started from the reference's graph after its inner phase, which no tie of the inner phase can reach."""
    from bayesiannetwork_amd.learning import BruteForce, Greedy, Learner, StepwiseStructure, structure_model
    table, runs = RL.load(name)
    run, t = runs[index], tables(name)
    plan = RL.plan_of(run)
    segments = RL.stepwise_segments(run)
    merges = []   # (parents, children, orders, the graph after the merge)
    for s, seg in enumerate(segments):
        end_graph = run.evals[segments[s + 1][3]][0] if s + 1 < len(segments) else RL.edge_set(run.final)
        if seg[0] == "between":
            merges.append((seg[1], seg[2], RL.orders_of(RL.try_segment(table.n, run.evals, seg[3], seg[4], end_graph)), end_graph))
    after_inner = RL.parents_of(table.n, run.evals[run.between_calls[0][2]][0])
    B = LR.reference_bound(table, run.final, run.criterion)

    class LoggedGreedy(Greedy):
        step = 0

        def hint_on(self, L, parent_nodes, child_nodes, orders=None):
            ps, cs, logged, _ = merges[self.step]
            assert (list(parent_nodes), list(child_nodes)) == (ps, cs)
            self.step += 1
            return super().hint_on(L, parent_nodes, child_nodes, orders=logged)

    # (2) first: it is the stricter one
    with Learner(t, after_inner, run.criterion) as L:
        greedy = Greedy(run.criterion, t)
        for ps, cs, logged, end_graph in merges:
            greedy.hint_on(L, ps, cs, orders=logged)
            assert RL.edge_set(L.parents()) == end_graph
        assert L.parents() == run.final and abs(L.score() - run.value) <= B
    # (1)
    between = LoggedGreedy(run.criterion, t)
    sw = StepwiseStructure(run.criterion, t, inner=BruteForce, between=between)
    start = structure_model(table.k, np.zeros(table.n + 1, np.int32), np.zeros(0, np.int32))
    learned, score = sw(start, run.size, plan=plan)
    assert between.step == len(merges) and sw.last_plan == ([list(c) for c in plan[0]], list(plan[1]))
    got = [learned.parents(v).tolist() for v in range(table.n)]
    with Learner(t, None, run.criterion) as L:   # the inner phase alone: the reference's graph, or per cluster an exactly tied twin
        for cluster in plan[0]:
            L.brute_force(cluster)
        inner = L.parents()
    assert inner == after_inner or RL.exact_tie(table, inner, after_inner), (inner, after_inner)
    print(f"{name} {run!r}: inner phase ends in the reference's graph: {inner == after_inner}; final graph equal: {got == run.final}")
    if inner == after_inner:
        assert got == run.final and abs(score - run.value) <= B
