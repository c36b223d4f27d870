"""The CPU side of structure learning (tests/learning_refs.py, bayesiannetwork_amd.learning): the restatement's greedy against the
literal reference loop, K2's cycle and precondition rules, the margin condition every input of the GPU test has to meet
(contract 5 of the header's learning section: a decision is only comparable across implementations when its margin exceeds the
sum of the two graphs' bounds -- required here with three orders of head-room), and the argument checks that need no device."""
import numpy as np
import pytest

import learning_refs as LR
import loglik_refs as R
from bayesiannetwork_amd import _lib, synth
from bayesiannetwork_amd.flat import FlatModel
from pattern_refs import fit_cpt_ref, random_patterns


def fitted(k, parents, pats, counts):
    from bayesiannetwork_amd.learning import structure_model
    ptr = np.zeros(len(k) + 1, dtype=np.int32)
    idx = []
    for v, ps in enumerate(parents):
        idx.extend(sorted(ps))
        ptr[v + 1] = len(idx)
    m = structure_model(k, ptr, np.asarray(idx, dtype=np.int32))
    m.cpt[:] = fit_cpt_ref(m, pats, counts)
    return m


def literal_greedy(k, pats, counts, criterion, orders, start=None):
    """greedy.hpp:26-62 with make_cpt + eval_ per candidate: eval_ is loglik_refs.reference_aic / reference_mdl (the reference's own
    likelihood loop over a dict of the table), add_edge's refusals are graph.hpp's."""
    ev = R.reference_aic if criterion == "aic" else R.reference_mdl
    table = R.table_dict(pats, counts)
    parents = [list(p) for p in (start or LR.empty_graph(len(k)))]
    now = ev(fitted(k, parents, pats, counts), table)
    edges = []
    for child, tail in zip(*orders):
        for u in tail:
            if u == child or u in parents[child] or u in LR.reaches(parents, child):
                continue
            parents[child].append(u)
            nxt = ev(fitted(k, parents, pats, counts), table)
            if nxt < now:
                now = nxt
                edges.append((u, child))
            else:
                parents[child].remove(u)
    return edges, now


def edges_of(parents):
    return sorted((u, v) for v, ps in enumerate(parents) for u in ps)


def small_inputs():
    pearl = synth.pearl()
    rng = np.random.default_rng(3)
    import exact_refs
    pats = np.array([exact_refs.forward_sample(pearl, rng) for _ in range(400)], dtype=np.uint8)
    yield "pearl", pearl.k, pats, np.ones(400, np.uint64)
    dag = synth.random_dag(12, 3, 6, [2, 3, 2, 4], seed=6)
    pats = np.array([exact_refs.forward_sample(dag, rng) for _ in range(1500)], dtype=np.uint8)
    yield "dag12", dag.k, pats, rng.integers(1, 4, 1500).astype(np.uint64)


@pytest.mark.parametrize("criterion", ["aic", "mdl"])
def test_restated_greedy_equals_the_literal_reference_loop(criterion):
    for name, k, pats, counts in small_inputs():
        table = LR.Table(pats, counts, k)
        for seed in (1, 2):
            orders = LR.greedy_orders(range(len(k)), seed)
            L = LR.RefLearner(k, LR.empty_graph(len(k)), criterion, table.total, table.libm_ll, record=True)
            LR.run_greedy(L, orders)
            edges, score = literal_greedy(k, pats, counts, criterion, orders)
            assert edges_of(L.parents) == sorted(edges), name
            assert len(edges) > 0
            # the two scores add the same terms in different orders
            assert abs(L.score - score) <= 2 * LR.graph_bound(table, L.parents, criterion), name
            # and the restated family term of a fitted model is bn_score_nodes' restatement, bit for bit
            m = fitted(k, L.parents, pats, counts)
            want = R.nodes_ref(m, R.family_counts_ref(m, pats, counts))
            assert [table.libm_ll(v, L.parents[v]) for v in range(len(k))] == want.tolist(), name
            assert L.score == LR.score_arith(want, R.parameters_ref(m), criterion, table.total), name


def test_family_counts_in_the_fitted_layout_and_every_insertion_position():
    k = [3, 2, 4, 2, 5]
    pats = random_patterns(k, 300, seed=1)
    counts = np.random.default_rng(2).integers(1, 1 << 40, 300).astype(np.uint64)
    for child, parents in ((4, []), (4, [2]), (2, [0, 4]), (1, [0, 3, 4]), (3, [0, 1, 2, 4])):
        ptr, idx = [0], []
        for v in range(len(k)):
            idx += parents if v == child else []
            ptr.append(len(idx))
        from bayesiannetwork_amd.learning import structure_model
        m = structure_model(k, np.asarray(ptr, np.int32), np.asarray(idx, np.int32))
        want = R.family_counts_ref(m, pats, counts)[int(m.cpt_off[child]):int(m.cpt_off[child + 1])]
        got = LR.family_counts(pats, counts, k, child, list(reversed(parents)))
        assert np.array_equal(got, want)
        assert int(got.sum(dtype=np.uint64)) == int(counts.sum(dtype=np.uint64))


def test_k2_refuses_a_cycle_and_honours_the_precondition():
    k = [2, 2, 2, 2]
    rng = np.random.default_rng(5)
    a = rng.integers(0, 2, 3000)
    b = a ^ (rng.random(3000) < 0.1)
    c = b ^ (rng.random(3000) < 0.1)
    d = rng.integers(0, 2, 3000)
    pats = np.stack([a, b, c, d], axis=1).astype(np.uint8)
    table = LR.Table(pats, np.ones(3000, np.uint64), k)
    start = [[], [0], [1], []]                      # 0 -> 1 -> 2
    L = LR.RefLearner(k, start, "mdl", table.total, table.libm_ll, record=True)
    got = L.try_parents(0, [2, 3])                  # 2 -> 0 would close 0 -> 1 -> 2 -> 0: never evaluated
    assert got == [False, False] and [d[1] for d in L.decisions] == [3]
    assert L.try_parents(2, [2, 1]) == [False, False] and len(L.decisions) == 1   # itself; already a parent
    # K2 over every target: strongly dependent 0 - 1 - 2 stay a DAG, the independent node 3 gets no edge
    L = LR.RefLearner(k, start, "mdl", table.total, table.libm_ll, record=True)
    LR.run_k2(L, [2, 0, 3, 1])
    left = {v: set(p) for v, p in enumerate(L.parents)}
    while left:                                      # acyclic: a topological order exists
        free = [v for v, p in left.items() if not p]
        assert free
        for v in free:
            del left[v]
        for p in left.values():
            p.difference_update(free)
    assert L.parents[3] == [] and all(3 not in p for p in L.parents)
    # precondition {2: [1]}: 1 may not become a parent of 2, so from an empty graph the edge 1 -> 2 is never tried
    L = LR.RefLearner(k, LR.empty_graph(4), "mdl", table.total, table.libm_ll, record=True)
    flags = LR.run_k2(L, [2, 1, 0, 3], {2: [1]})
    assert 1 not in flags[0][0] and (2, 1) not in [(d[0], d[1]) for d in L.decisions]
    assert 1 not in L.parents[2]
    # ... and an accepted parent never gets its child as a candidate later (k2_algorithm.hpp:57)
    targets = [2, 1, 0, 3]
    for (cand, got), target in zip(flags, targets):
        for u, ok in zip(cand, got):
            if ok and targets.index(u) > targets.index(target):
                assert target not in flags[targets.index(u)][0]
    assert sum(len(p) for p in L.parents) >= 2


def test_max_parents_and_limits_stop_the_scan():
    k = [2] * 6
    pats = random_patterns(k, 64, seed=3)
    pats[:, 5] = pats[:, 0] ^ pats[:, 1] ^ pats[:, 2] ^ pats[:, 3]
    table = LR.Table(pats, np.full(64, 50, np.uint64), k)
    L = LR.RefLearner(k, LR.empty_graph(6), "aic", table.total, table.libm_ll, max_parents=2)
    L.try_parents(5, [0, 1, 2, 3, 4])
    assert len(L.parents[5]) <= 2


@pytest.mark.parametrize("name", LR.INPUT_NAMES)
def test_margin_condition_on_the_inputs_of_the_gpu_test(name):
    """Contract 5 is a condition on the input: every decision of the public-API loop (restated with libm) must be decided by
    more than the two graphs' bounds.  Required: margin > 1000 x bound for EVERY decision (share left out: zero)."""
    model, table, criterion, orders, max_parents = LR.learning_input(name)
    L = LR.RefLearner(model.k, LR.empty_graph(model.n), criterion, table.total, table.libm_ll, max_parents, record=True)
    LR.run_greedy(L, orders)
    ms = LR.margins(table, L)
    worst = min(ms, key=lambda x: x[0] / x[1])
    smallest = min(ms, key=lambda x: x[0])
    print(f"{name}: {len(ms)} decisions, {sum(len(p) for p in L.parents)} accepted, smallest margin {smallest[0]:.3g} "
          f"(bound there {smallest[1]:.3g}), smallest margin / bound {worst[0] / worst[1]:.3g}")
    n = model.n
    assert len(ms) <= n * (n - 1) // 2 and len(ms) > n * (n - 1) // 4
    assert sum(len(p) for p in L.parents) > 0
    for margin, bound in ms:
        assert margin > 1000 * bound


@pytest.mark.parametrize("kind", ["hint", "k2"])
def test_margin_condition_on_the_hint_and_k2_inputs(kind):
    model, table, criterion, _, max_parents = LR.learning_input("alarm2k_mdl")
    L = LR.RefLearner(model.k, LR.empty_graph(model.n), criterion, table.total, table.libm_ll, max_parents, record=True)
    if kind == "hint":
        LR.run_hint(L, LR.hint_orders(model.n, 31))
    else:
        LR.run_k2(L, LR.k2_children(model.n, 41), LR.K2_PRECONDITION)
    ms = LR.margins(table, L)
    print(f"{kind}: {len(ms)} decisions, {sum(len(p) for p in L.parents)} accepted, smallest margin / bound "
          f"{min(m / b for m, b in ms):.3g}")
    assert len(ms) > 100 and sum(len(p) for p in L.parents) > 0
    for margin, bound in ms:
        assert margin > 1000 * bound


def test_argument_checks_that_need_no_device(bnlib):
    from bayesiannetwork_amd import Greedy, K2, Learner, score_groups   # noqa: F401  (exported)
    from bayesiannetwork_amd import learning
    import ctypes
    lib = _lib.lib()
    one = np.zeros(2, dtype=np.int32)
    ll = np.zeros(1)
    p32 = lambda a: a.ctypes.data_as(_lib.i32p)   # noqa: E731
    assert lib.bn_learn_score_groups(None, 0, None, None, None, None, None, ll.ctypes.data_as(_lib.f64p), None) == _lib.BN_ERR_ARG
    h = ctypes.c_void_p()
    assert lib.bn_learn_create(None, p32(one), None, 0, 4, ctypes.byref(h)) == _lib.BN_ERR_ARG and not h.value
    out = ctypes.c_double()
    assert lib.bn_learn_score(None, ctypes.byref(out)) == _lib.BN_ERR_ARG
    assert lib.bn_learn_try_parents(None, 0, 0, None, None) == _lib.BN_ERR_ARG
    assert lib.bn_learn_structure(None, p32(one), None) == _lib.BN_ERR_ARG
    v = ctypes.c_int64()
    assert lib.bn_learn_get(None, b"passes", ctypes.byref(v)) == _lib.BN_ERR_ARG
    lib.bn_learn_destroy(None)
    assert b"null" in lib.bn_last_error()
    with pytest.raises(ValueError):
        learning._criterion("bic")
    from bayesiannetwork_amd.evaluation import AIC, MDL
    assert learning._criterion("AIC") == 0 and learning._criterion(MDL) == 1 and learning._criterion(AIC(None)) == 0
    m = learning.structure_model([2, 3, 4], np.array([0, 0, 1, 3], np.int32), np.array([0, 0, 1], np.int32))
    assert isinstance(m, FlatModel) and m.cpt_off.tolist() == [0, 2, 8, 32]
    m.validate()
