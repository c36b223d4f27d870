"""CPT fitting, AIC / MDL and the structure searches pinned to the REFERENCE'S OWN CODE on the CPU: tests/golden/learn_*.npz hold
what the unmodified sampler.hpp, evaluation/{aic,mdl}.hpp and learning/{greedy,k2_algorithm,brute_force,stepwise_structure}.hpp
did (oracle/ref_learn_driver.cpp; tests/golden/make_golden.py --learning), and the project's restatements -- learning_refs,
subset_refs, oracle_make_cpt -- are held against them here.  Every check runs over every fixture, every run and every logged
evaluation; nothing is sampled."""
import math

import numpy as np
import pytest

import learning_refs as LR
import reference_learning as RL
import subset_refs as SR

FIXTURES = RL.fixture_names()


def ids(pairs):
    return [f"{name}-{i}-{RL.load(name)[1][i]!r}" for name, i in pairs]


def cases(kinds):
    pairs = RL.all_runs(kinds)
    return pytest.mark.parametrize("name,index", pairs, ids=ids(pairs))


def searcher(table, run, start=None):
    return SR.RefSearch(table.k, run.start if start is None else start, run.criterion, table.total, table.libm_ll)


def test_the_fixtures_are_the_ones_the_generator_writes():
    assert set(FIXTURES) == {"n5", "n6", "bd12", "alarm2k_mdl"}
    for name in FIXTURES:
        table, runs = RL.load(name)
        _, specs = RL.run_specs(name)
        assert [(r.kind, r.criterion or None, r.seed, r.start) for r in runs] == [(s["kind"], s["criterion"], s["seed"], s["start"]) for s in specs]
        assert np.array_equal(table.pats, RL.input_table(name).pats) and np.array_equal(table.counts, RL.input_table(name).counts)


# ---- make_cpt ------------------------------------------------------------------------------------------------------

def restated_cpt(table, parents):
    """theta = double(N) / double(row total); 1.0 / k for a row no sample shows (sampler.hpp:141-156)."""
    out = []
    for v in range(table.n):
        kv = int(table.k[v])
        N = LR.family_counts(table.pats, table.counts, table.k, v, parents[v]).reshape(-1, kv)
        for row in N:
            tot = int(row.sum(dtype=np.uint64))
            out.extend([1.0 / kv] * kv if tot == 0 else [float(int(x)) / float(tot) for x in row])
    return np.array(out)


@cases(("make_cpt",))
def test_the_restated_make_cpt_has_the_references_bits(name, index, oracle_mod):
    from bayesiannetwork_amd.learning import structure_model
    table, runs = RL.load(name)
    run = runs[index]
    want = run.cpt
    got = restated_cpt(table, run.start)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    ptr, idx = RL._ragged(run.start, np.int32)
    model = structure_model(table.k, ptr, idx)
    c = oracle_mod.make_cpt(model, table.pats, table.counts)   # the C restatement the GPU tests of fit_cpt compare with
    assert np.array_equal(c.view(np.uint64), want.view(np.uint64))


def test_a_make_cpt_fixture_has_unseen_parent_configurations():
    seen = 0
    for name, index in RL.all_runs(("make_cpt",)):
        table, runs = RL.load(name)
        run = runs[index]
        for v in range(table.n):
            N = LR.family_counts(table.pats, table.counts, table.k, v, run.start[v]).reshape(-1, int(table.k[v]))
            rows = np.nonzero(N.sum(axis=1) == 0)[0]
            if len(rows):
                seen += len(rows)
                off = sum(int(table.k[u]) * math.prod(int(table.k[x]) for x in run.start[u]) for u in range(v))
                for r in rows:
                    assert np.all(run.cpt[off + r * int(table.k[v]):off + (r + 1) * int(table.k[v])] == 1.0 / int(table.k[v]))
    assert seen >= 10


# ---- scores ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_every_logged_score_is_the_restated_one_within_the_derived_bound(name):
    """|reference's aic / mdl - score_arith over Table.libm_ll| <= reference_bound at EVERY logged evaluation.  graph_bound's
    own derivation (one computation in a stated order) does not cover the reference's single running sum over all M terms in
    hash order; reference_bound adds that computation's gamma_{M+2} (learning_refs.reference_bound's text)."""
    table, runs = RL.load(name)
    worst, count, over_graph_bound = 0.0, 0, 0
    for run in runs:
        if run.kind == "make_cpt":
            continue
        for es, vs, value in run.evals:
            parents = RL.parents_of(table.n, es)
            mine = RL.restated_value(table, parents, run.criterion, vs)
            B = LR.reference_bound(table, parents, run.criterion, vs)
            assert abs(mine - value) <= B, (run, sorted(es), vs, mine, value, B)
            worst = max(worst, abs(mine - value) / B)
            over_graph_bound += vs is None and abs(mine - value) > LR.graph_bound(table, parents, run.criterion)
            count += 1
        assert run.value in [v for _, _, v in run.evals]   # what a search returns is one of the values its Eval gave it
    print(f"{name}: {count} logged evaluations, largest |difference| / bound {worst:.3g}; {over_graph_bound} beyond graph_bound")
    assert count > 0


def test_the_score_runs_cover_both_forms_and_the_vertex_list_form_counts_only_its_vertexes():
    forms = set()
    for name, index in RL.all_runs(("score",)):
        table, runs = RL.load(name)
        run = runs[index]
        (es, vs, value), = run.evals
        assert es == RL.edge_set(run.start) and vs == run.vertexes and value == run.value
        forms.add((run.criterion, vs is None))
        if vs is not None:   # the whole graph's likelihood is far outside the bound: the other nodes' terms are NOT in it
            whole = RL.restated_value(table, run.start, run.criterion)
            assert abs(whole - value) > 1000 * LR.reference_bound(table, run.start, run.criterion)
    assert forms == {("aic", True), ("aic", False), ("mdl", True), ("mdl", False)}


# ---- the decisions a log holds -----------------------------------------------------------------------------------------

def log_decisions(table, run):
    """Every decision of a run as (margin, sum of the two bounds, what it was, the two graphs, the vertex list): candidates
    against eval_now, leaves against best_eval, from the reference's own logged values."""
    n, c = table.n, run.criterion

    def tries(begin, end, end_graph):
        out = []
        for child, u, value, now, kept, before in RL.try_segment(n, run.evals, begin, end, end_graph):
            assert kept == (value < now), (run, child, u)   # (greedy.hpp:47, k2_algorithm.hpp:54: strictly smaller)
            after = [list(p) for p in before]
            after[child] = sorted(after[child] + [u])
            out.append((abs(value - now), LR.reference_bound(table, after, c) + LR.reference_bound(table, before, c), (child, u), after, before, None))
        return out

    def leaves(begin, end):
        out = []
        best_g, vs, best = run.evals[begin]
        for es, vs2, value in run.evals[begin + 1:end]:
            assert vs2 == vs
            if es == best_g:
                assert value == best   # the same graph again: the same bits, so `<` does not take it
            else:
                g, b = RL.parents_of(n, es), RL.parents_of(n, best_g)
                out.append((abs(value - best), LR.reference_bound(table, g, c, vs) + LR.reference_bound(table, b, c, vs), sorted(es), g, b, vs))
            if value < best:
                best_g, best = es, value
        return out, best_g, best
    if run.kind in RL.TRY_KINDS:
        return tries(0, len(run.evals), RL.edge_set(run.final))
    if run.kind in RL.BRUTE_KINDS:
        out, best_g, best = leaves(0, len(run.evals))
        assert best_g == RL.edge_set(run.final) and best == run.value
        return out
    out, segments = [], RL.stepwise_segments(run)
    for s, seg in enumerate(segments):
        end_graph = run.evals[segments[s + 1][3]][0] if s + 1 < len(segments) else RL.edge_set(run.final)
        if seg[0] == "inner":
            got, best_g, _ = leaves(seg[3], seg[4])
            assert best_g == end_graph
            out += got
        else:
            out += tries(seg[3], seg[4], end_graph)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_every_logged_decision_is_decided_by_more_than_1000_bounds_or_is_an_exact_tie(name):
    """Contracts 4 and 5 on the fixtures: at every decision the reference took -- a candidate against eval_now, a leaf against
    best_eval -- the margin exceeds 1000 x the sum of the two graphs' bounds, so the restatements and the device can be asked
    for the SAME decisions with none left out.

    One class of decisions cannot meet that on any input or seed, and the inputs fixed for these fixtures contain it by
    construction: comparisons of two graphs whose scores are EQUAL in exact arithmetic.  AIC and MDL are score equivalent, and
    brute_force compares a -> b with b -> a at every level (so does stepwise_structure's inner learning); an edge at n6's node
    of arity 1 changes neither the likelihood nor the parameter count.  As the condition was first written -- every decision
    above 1000 bounds -- it failed on n5 (36 of 6 213 decisions), n6 (144 of 558) and bd12 (10 of 627), every one of them with a
    margin of 0 or of a few 1e-12 on scores of 1e4.  Such a pair is recognised here WITHOUT floating point (RL.exact_tie: equal
    parameter counts and the same signed multiset of N log N terms); for it the test demands what can be demanded: the two
    computed values differ by no more than the two bounds.  Every other decision must clear 1000 bounds; a seed at which one
    does not is replaced in tests/reference_learning.py, not excused here."""
    table, runs = RL.load(name)
    smallest, count, ties, failures = math.inf, 0, 0, []
    for run in runs:
        if run.kind in ("make_cpt", "score"):
            continue
        for margin, bound, what, a, b, vs in log_decisions(table, run):
            count += 1
            if margin > 1000 * bound:
                smallest = min(smallest, margin / bound)
            elif RL.exact_tie(table, a, b, vs):
                ties += 1
                assert margin <= bound, (repr(run), what, margin, bound)
            else:
                failures.append((repr(run), what, margin, bound))
    print(f"{name}: smallest margin / bound over {count - ties} decisions: {smallest:.3g}; {ties} exact ties")
    assert count > ties and not failures, (len(failures), failures[:5])
    assert (ties > 0) == (name != "alarm2k_mdl")   # greedy from no edges on arities >= 2 compares no two equivalent graphs


# ---- the restatements take the reference's decisions -----------------------------------------------------------------------

@cases(RL.TRY_KINDS)
def test_the_restated_loops_take_the_references_decisions(name, index):
    table, runs = RL.load(name)
    run = runs[index]
    decisions = RL.try_segment(table.n, run.evals, 0, len(run.evals), RL.edge_set(run.final))
    assert run.evals[0][0] == RL.edge_set(run.start)
    children, tails = RL.orders_of(decisions)
    want = [(c, p, kept) for c, p, _, _, kept, _ in decisions]
    L = LR.RefLearner(table.k, run.start, run.criterion, table.total, table.libm_ll, record=True)
    if run.kind == "k2":
        assert len(set(children)) == len(children)
        order = children + [v for v in range(table.n) if v not in children]   # a target none of whose candidates could be added
        flags = LR.run_k2(L, order, run.precondition)
        logged = {(c, p) for c, p, _ in want}
        for target, (cand, got) in zip(order, flags):
            assert target not in cand and not set(cand) & set(run.precondition.get(target, ()))
            for u, ok in zip(cand, got):
                assert (target, u) in logged or not ok   # a candidate the reference did not evaluate was refused by add_edge
    else:
        LR.run_greedy(L, (children, tails))
    got = [(c, u, take) for c, u, _, _, take, _ in L.decisions]
    assert got == want                                                    # the same candidates evaluated, the same accept flags
    assert L.parents == run.final
    assert abs(L.score - run.value) <= LR.reference_bound(table, run.final, run.criterion)
    assert len(decisions) > 0 and any(k for _, _, k in want)


@cases(RL.BRUTE_KINDS)
def test_the_restated_enumerations_visit_the_references_leaves_in_its_order(name, index):
    table, runs = RL.load(name)
    run = runs[index]
    L = searcher(table, run)
    if run.kind == "brute_hint":
        vs = None
        best, ev, leaves = SR.literal_hint(L, *run.hint)
    else:
        vs = list(range(table.n)) if run.kind == "brute_all" else run.vertexes
        best, ev, leaves = SR.literal_brute_force(L, vs)
    assert run.evals[0][:2] == (RL.edge_set(run.start), vs)
    assert [RL.edge_set(g) for g, _ in leaves] == [es for es, _, _ in run.evals[1:]]   # the same leaves in the same order
    assert all(v == vs for _, v, _ in run.evals)
    assert best == run.final
    B = LR.reference_bound(table, run.final, run.criterion, vs)
    assert abs(ev - run.value) <= B
    # the return value: the likelihood over `vertexes` ONLY, the parameters of the WHOLE graph
    assert abs(RL.restated_value(table, run.final, run.criterion, vs) - run.value) <= B
    if vs is not None and len(vs) < table.n:
        assert abs(RL.restated_value(table, run.final, run.criterion) - run.value) > 1000 * LR.reference_bound(table, run.final, run.criterion)
    # the library's restatement (the enumeration without the repeated branches; the decomposed hint search) ends there too
    M = searcher(table, run)
    got = M.brute_force_hint(*run.hint) if run.kind == "brute_hint" else M.brute_force(vs)
    assert M.parents == run.final and got == ev


@cases(("stepwise",))
def test_the_restated_stepwise_search_follows_the_references_calls(name, index):
    table, runs = RL.load(name)
    run = runs[index]
    clusters, pairs = RL.plan_of(run)
    assert sorted(v for c in clusters for v in c) == list(range(table.n))
    assert len(clusters) == -(-table.n // run.size) and max(len(c) for c in clusters) - min(len(c) for c in clusters) <= 1   # (:47-61)
    assert len(pairs) == len(clusters) - 1
    L = searcher(table, run, LR.empty_graph(table.n))   # (:26: the edges are erased first)
    segments, exact = RL.stepwise_segments(run), 0
    for s, seg in enumerate(segments):
        begin, end = seg[3], seg[4]
        end_graph = run.evals[segments[s + 1][3]][0] if s + 1 < len(segments) else RL.edge_set(run.final)
        assert run.evals[begin][0] == RL.edge_set(L.parents)
        if seg[0] == "inner":
            best, _, leaves = SR.literal_brute_force(L, seg[1])
            assert [RL.edge_set(g) for g, _ in leaves] == [es for es, _, _ in run.evals[begin + 1:end]]
            assert all(v == seg[1] for _, v, _ in run.evals[begin:end])
            # the enumeration compares a -> b with b -> a: equal in exact arithmetic, settled by each side's own rounding.  The
            # restated best is the reference's, or exactly tied with it; the replay goes on from the reference's choice
            theirs = RL.parents_of(table.n, end_graph)
            assert best == theirs or RL.exact_tie(table, best, theirs, seg[1]), (seg[1], best, theirs)
            exact += best == theirs
            L._set(theirs)
        else:
            decisions = RL.try_segment(table.n, run.evals, begin, end, end_graph)
            children, cands = RL.orders_of(decisions)
            assert set(children) <= set(seg[2]) and all(set(c) <= set(seg[1]) for c in cands)
            flags = LR.run_hint(L, (children, cands))
            assert [bool(f) for fs in flags for f in fs] == [kept for *_, kept, _ in decisions]
        assert RL.edge_set(L.parents) == end_graph
    assert L.parents == run.final and exact > 0
    assert abs(L.score - run.value) <= LR.reference_bound(table, run.final, run.criterion)


# ---- greedy's orders ------------------------------------------------------------------------------------------------------

@cases(("greedy_all", "greedy_vertexes", "greedy_hint"))
def test_the_orders_in_the_log_are_accumulating_shuffles(name, index):
    """greedy.hpp:28-37: ONE vector is shuffled, then its tail after every child again, so child i + 1 is the head of tail i and
    tail i + 1 a permutation of the rest of tail i.  learn_with_hint (:70-80) shuffles the one parent vector per child."""
    table, runs = RL.load(name)
    run = runs[index]
    decisions = RL.try_segment(table.n, run.evals, 0, len(run.evals), RL.edge_set(run.final))
    children, tails = RL.orders_of(decisions)
    if run.kind == "greedy_hint":
        ps, cs = run.hint
        assert len(set(children)) == len(children) and set(children) <= set(cs)
        if not any(run.start):   # no edge to begin with and parents apart from children: nothing is refused, all are logged
            assert sorted(children) == sorted(cs) and all(sorted(t) == sorted(ps) for t in tails)
        return
    nodes = list(range(table.n)) if run.kind == "greedy_all" else run.vertexes
    if not any(run.start):       # from no edges every edge of a tail can be added: the log shows the orders completely
        assert len(children) == len(nodes) - 1 and sorted(children + tails[-1]) == sorted(nodes)
        assert sorted(tails[0] + [children[0]]) == sorted(nodes)
    for i in range(len(children) - 1):
        if not any(run.start):
            assert children[i + 1] == tails[i][0] and sorted(tails[i + 1]) == sorted(tails[i][1:])
        else:                    # refused candidates are missing from the log: what is there must still fit such an order
            assert children[i + 1] not in children[:i + 1] and set(tails[i + 1]) <= set(nodes) - set(children[:i + 2])
    # the project's own orders accumulate the same way (learning.Greedy.run_on without `orders`, learning_refs.greedy_orders' reading)
    assert all(c not in t for c, t in zip(children, tails))


# ---- regeneration -----------------------------------------------------------------------------------------------------------

def test_regenerating_the_quickest_fixture_reproduces_the_committed_arrays(oracle_mod):
    if not oracle_mod.ref_learn_available():
        pytest.skip("oracle/_ref/ref_learn_driver is built only where the reference is present")
    name = "n6"
    z = np.load(f"{RL.GOLDEN}/learn_{name}.npz")
    table, specs = RL.run_specs(name)
    assert int(z["n_runs"]) == len(specs)
    for i, spec in enumerate(specs):
        out = oracle_mod.ref_learn(table.k, spec["start"], table.pats, table.counts, RL.command_of(spec))
        for key, val in RL.pack_run(spec, out).items():
            want = z[f"run{i}_{key}"]
            assert want.dtype == np.asarray(val).dtype and np.array_equal(want, val), (i, key)
