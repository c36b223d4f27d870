"""CPU checks under tests/test_subsets_gpu.py: the restatement of the exhaustive searches (tests/subset_refs.py) against a literal
transcription of the reference's recursions, the lattice's index arithmetic against direct counting, and the MARGIN CONDITION on
every hint search the GPU test compares with the public-API loop: the best graph of the search differs from every other graph it
visits by more than 1000 x the sum of the two graphs' bounds B (learning_refs.graph_bound), so equal edges can be demanded."""
import ctypes
import itertools

import numpy as np
import pytest

import learning_refs as LR
import subset_refs as SR
from bayesiannetwork_amd import _lib


def small_table(seed, n=7, rows=400):
    """Columns with real dependencies: 2 <- 0 xor 1 (noisy), 4 <- 3 (noisy copy), 5 <- 2 and 4, 6 free; arities 2 and 3."""
    r = np.random.default_rng(seed)
    k = [2, 2, 2, 3, 3, 2, 2][:n]
    pats = np.zeros((rows, n), np.uint8)
    pats[:, 0], pats[:, 1], pats[:, 3], pats[:, 6] = r.integers(0, 2, rows), r.integers(0, 2, rows), r.integers(0, 3, rows), r.integers(0, 2, rows)
    pats[:, 2] = (pats[:, 0] ^ pats[:, 1]) ^ (r.random(rows) < 0.1)
    pats[:, 4] = np.where(r.random(rows) < 0.85, pats[:, 3], r.integers(0, 3, rows))
    pats[:, 5] = ((pats[:, 2] + pats[:, 4]) % 2) ^ (r.random(rows) < 0.15)
    return LR.Table(pats, r.integers(1, 5, rows).astype(np.uint64), k)


def searcher(table, parents, criterion, max_parents=LR.MAX_PARENTS):
    return SR.RefSearch(table.k, parents, criterion, table.total, table.libm_ll, max_parents)


def test_the_lattice_arithmetic_gives_the_counts_of_every_subset():
    r = np.random.default_rng(3)
    k = [2, 3, 1, 4, 2, 5, 3, 2]
    pats = np.stack([r.integers(0, kk, 500) for kk in k], axis=1).astype(np.uint8)
    counts = r.integers(1, 1 << 40, 500).astype(np.uint64)
    for child, base, cand in ((7, [], [0, 1, 2]), (0, [3], [5, 1, 2, 6]), (4, [1, 6], [0, 7, 3]), (2, [0, 7], [4]), (5, [2], [])):
        top = LR.family_counts(pats, counts, k, child, base + cand)
        got = SR.lattice_counts(top, k, child, base, cand)
        assert len(got) == 1 << len(cand)
        for mask, N in enumerate(got):
            S = [cand[j] for j in range(len(cand)) if (mask >> j) & 1]
            assert np.array_equal(N, LR.family_counts(pats, counts, k, child, base + S)), (child, base, S)


def test_the_visiting_order_is_mask_order_with_the_bits_reversed():
    assert SR.visiting_order(0) == [0] and SR.visiting_order(1) == [0, 1]
    assert SR.visiting_order(3) == [0, 4, 2, 6, 1, 5, 3, 7]   # cand[2] toggles fastest, cand[0] slowest


STARTS = [
    [[], [], [], [], [], [], []],
    [[], [], [0], [], [3], [], []],            # existing edges inside the sets: refused as duplicates, their reverses as cycles
    [[2], [], [], [], [], [4], [5]],           # 2 -> 0, 4 -> 5 -> 6
]


@pytest.mark.parametrize("criterion", ["aic", "mdl"])
def test_the_restated_hint_search_is_the_literal_recursion(criterion):
    table = small_table(1)
    decomposed = literal = 0
    for start, (par, child), max_parents in itertools.product(
            STARTS, (([0, 1, 3], [2, 4, 5]), ([0, 1, 2, 4], [5, 6]), ([2, 4, 0], [0, 5, 6]), ([5, 6], [2, 4]), ([0, 0, 1], [2, 2]), ([3], [])),
            (LR.MAX_PARENTS, 2)):
        a, b = searcher(table, start, criterion, max_parents), searcher(table, start, criterion, max_parents)
        want_graph, want_score, leaves = SR.literal_hint(a, par, child)
        if b.decomposes(par, child):
            decomposed += 1
        else:
            literal += 1
        got_score = b.brute_force_hint(par, child)
        assert b.parents == want_graph and got_score == want_score, (start, par, child)
        assert all(len(p) <= max(max_parents, max(len(q) for q in start)) for p in b.parents)
        assert any(g == want_graph for g, _ in leaves)
    assert decomposed >= 8 and literal >= 8   # both ways are exercised


@pytest.mark.parametrize("criterion", ["aic", "mdl"])
def test_the_restated_enumeration_is_the_literal_recursion(criterion):
    table = small_table(2)
    for start, vs, max_parents in itertools.product(STARTS, ([2, 0, 1], [5, 2, 4, 3], [6, 5, 4, 2, 0], [4], [], [3, 4]), (LR.MAX_PARENTS, 1)):
        a, b = searcher(table, start, criterion, max_parents), searcher(table, start, criterion, max_parents)
        want_graph, want_eval, leaves = SR.literal_brute_force(a, vs)
        got_eval = b.brute_force(vs)
        assert b.parents == want_graph and got_eval == want_eval, (start, vs)
        distinct = {tuple(tuple(p) for p in g) for g, _ in leaves}
        if len(vs) == 5 and not any(start) and max_parents == LR.MAX_PARENTS:
            assert len(leaves) == 12 * 9 * 6 * 3 and len(distinct) == 9 * 7 * 5 * 3   # (brute_force.hpp:139-154 repeats "no edge" per i)
    # the evaluated quantity: the likelihood over the vertexes IN THE GIVEN ORDER, the parameters of the whole graph
    L = searcher(table, STARTS[2], criterion)
    ll = [table.libm_ll(v, L.parents[v]) for v in (5, 2, 4)]
    assert L._score(L.parents, [5, 2, 4]) == LR.score_arith(ll, L.params, criterion, table.total)


@pytest.mark.parametrize("name", LR.INPUT_NAMES)
def test_margins_of_every_hint_search_the_gpu_test_compares(name):
    model, table, criterion, max_parents, calls = SR.hint_calls(name)
    L = SR.RefSearch(model.k, LR.empty_graph(model.n), criterion, table.total, table.libm_ll, max_parents)
    smallest, nonempty, literal = float("inf"), 0, 0
    assert len(calls) == SR.HINT_CHILDREN and all(len(p) == SR.HINT_CANDIDATES and len(c) == 1 for p, c in calls)
    for par, child in calls:
        twin = SR.RefSearch(model.k, L.parents, criterion, table.total, table.libm_ll, max_parents)
        best_graph, best, leaves = SR.literal_hint(twin, par, child)
        graphs = {tuple(tuple(p) for p in g): s for g, s in leaves}
        if not L.decomposes(par, child):
            literal += 1
        else:
            assert len(graphs) == 1 << SR.HINT_CANDIDATES   # every subset is there: none is left out of the comparison
        B_best = LR.graph_bound(table, best_graph, criterion)
        for g, s in graphs.items():
            if [list(p) for p in g] == best_graph:
                assert s == best
                continue
            ratio = abs(s - best) / (B_best + LR.graph_bound(table, [list(p) for p in g], criterion))
            smallest = min(smallest, ratio)
            assert s > best and ratio > 1000, (name, child, g[child[0]], ratio)
        assert L.brute_force_hint(par, child) == best and L.parents == best_graph   # (the restatement takes the literal's decision)
        nonempty += len(L.parents[child[0]]) > 0
    print(f"{name}: smallest margin / bound over {len(calls)} searches: {smallest:.3g}; {nonempty} children with parents; "
          f"{literal} searches with a refused edge")
    assert 2 * nonempty >= len(calls)


def test_argument_checks_that_need_no_device(bnlib):
    from bayesiannetwork_amd import BruteForce, StepwiseStructure, score_subsets   # noqa: F401  (exported)
    lib = _lib.lib()
    one = np.zeros(2, dtype=np.int32)
    ll = np.zeros(1)
    p32 = lambda a: a.ctypes.data_as(_lib.i32p)   # noqa: E731
    assert lib.bn_learn_score_subsets(None, 0, 0, None, 0, None, ll.ctypes.data_as(_lib.f64p), None) == _lib.BN_ERR_ARG
    assert b"null" in lib.bn_last_error()
    taken = np.zeros(2, dtype=np.uint8)
    assert lib.bn_learn_best_parents(None, 0, 1, p32(one), taken.ctypes.data_as(_lib.u8p)) == _lib.BN_ERR_ARG
    assert lib.bn_learn_terms(None, ll.ctypes.data_as(_lib.f64p), None) == _lib.BN_ERR_ARG
    assert lib.bn_learn_brute_force_hint(None, 1, p32(one), 1, p32(one)) == _lib.BN_ERR_ARG
    out = ctypes.c_double()
    assert lib.bn_learn_brute_force(None, 1, p32(one), ctypes.byref(out)) == _lib.BN_ERR_ARG
