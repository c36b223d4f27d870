"""bn_tree_max_spanning (Prim's algorithm in one workgroup) against tests/tree_refs.py's Kruskal under the same edge order, and the
learners on top of it: ChowLiu and TAN return the tree of the device's own weight matrix, recover a chain, and feed a Learner.

Sizes on either side of a wave (63, 64, 65), of four waves (257) and of the workgroup's 1024 threads (1025: some threads own two
nodes), and the trivial 1, 2, 3."""
import numpy as np
import pytest

import tree_refs as TR

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 257, 1025]


def roots(m):
    return sorted({0, m // 2, m - 1})


def matrices(m):
    """name -> w [m][m]; the lower triangle holds garbage (NaN and numbers that would change the tree): only the upper one is read."""
    rng = np.random.default_rng(100 + m)
    out = {
        "random": rng.standard_normal((m, m)),                                   # negative weights too
        "integers": rng.integers(-2, 3, (m, m)).astype(np.float64),              # heavy ties
        "equal": np.full((m, m), 0.25),
        "zeros": np.where(rng.random((m, m)) < 0.5, -0.0, 0.0),                  # -0.0 against 0.0: all equal under the order
    }
    special = rng.integers(-1, 2, (m, m)).astype(np.float64)
    special[rng.random((m, m)) < 0.1] = np.inf
    special[rng.random((m, m)) < 0.1] = -np.inf
    special[rng.random((m, m)) < 0.2] = -0.0
    out["special"] = special
    for name, w in out.items():
        low = np.tril_indices(m, -1)
        w[low] = np.where(rng.random(len(low[0])) < 0.5, np.nan, 1e6 * rng.standard_normal(len(low[0])))
        w[np.diag_indices(m)] = np.nan
    return out


@pytest.mark.parametrize("m", SIZES)
def test_equals_kruskal(bnlib, m):
    from bayesiannetwork_amd.learning import max_spanning_tree
    for name, w in matrices(m).items():
        edges = TR.kruskal_edges(w)
        for root in roots(m):
            got = max_spanning_tree(w, root, device=0)
            assert got.dtype == np.int32 and np.array_equal(got, TR.orient(m, edges, root)), (name, root)


def test_refusals(bnlib):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.learning import max_spanning_tree
    w = np.zeros((5, 5))
    for root in (-1, 5):
        with pytest.raises(_lib.BnError, match="root"):
            max_spanning_tree(w, root, device=0)
    bad = w.copy()
    bad[1, 3] = np.nan
    with pytest.raises(_lib.BnError, match="NaN"):
        max_spanning_tree(bad, 0, device=0)
    bad = w.copy()
    bad[3, 1] = np.nan                                                            # the lower triangle is not read
    assert np.array_equal(max_spanning_tree(bad, 0, device=0), TR.kruskal(w, 0))
    with pytest.raises(_lib.BnError, match="4096"):
        max_spanning_tree(np.zeros((4097, 4097)), 0, device=0)
    lib = _lib.lib()
    assert lib.bn_tree_max_spanning(5, None, 0, 0, None) == -1 and lib.bn_last_error().decode() != ""


def chain_table(n, P, k, seed, class_col=False):
    """Column i copies column i - 1 with probability 0.8, else it is uniform; with class_col, column 0 is a class every feature
    also follows with probability 0.1 and the chain starts at column 1."""
    rng = np.random.default_rng(seed)
    pats = np.zeros((P, n), np.uint8)
    pats[:, 0] = rng.integers(0, k, P)
    first = 1 if class_col else 0
    for c in range(first, n):
        col = rng.integers(0, k, P)
        if c > first:
            col = np.where(rng.random(P) < 0.8, pats[:, c - 1], col)
        if class_col:
            col = np.where(rng.random(P) < 0.1, pats[:, 0], col)
        pats[:, c] = col
    return pats, np.ones(P, np.uint64), np.full(n, k, np.int32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check_tree(r, matrix):
    """The result's tree is Kruskal's on the device's own matrix, and its weights are that matrix's entries."""
    v = [int(x) for x in r.variables]
    assert same_bits(r.matrix, matrix)
    want = TR.kruskal(r.matrix, v.index(r.root))
    assert np.array_equal(r.parent, [v[p] if p >= 0 else -1 for p in want])
    for i, p in enumerate(r.parent):
        assert same_bits(r.weight[i], r.matrix[i, v.index(int(p))] if p >= 0 else 0.0)


def test_chow_liu(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import ChowLiu, Learner, structure_model
    n = 24
    pats, counts, k = chain_table(n, 4000, 3, seed=7)
    with InfoTable(pats, counts, k, device=0) as t:
        r = ChowLiu()(t)
        check_tree(r, t.pair_entropies()["mi"])
        assert r.root == 0 and r.cond == -1 and t.info("tree_ns") > 0
        assert np.array_equal(r.parent, np.arange(-1, n - 1))                    # the chain
        assert r.parents() == [[]] + [[i - 1] for i in range(1, n)]
        mid = ChowLiu(root=11)(t)
        check_tree(mid, t.pair_entropies()["mi"])
        assert mid.root == 11 and mid.parents() == [[i + 1] for i in range(11)] + [[]] + [[i - 1] for i in range(12, n)]
        sub = [9, 3, 20, 4, 5, 21]                                               # a subset in another order: the lowest is the root
        rs = ChowLiu()(t, sub)
        check_tree(rs, t.pair_entropies(sub)["mi"])
        assert rs.root == 3 and rs.parents()[0] == [] and rs.parents()[4] == [3] and rs.parents()[5] == [4]
        assert same_bits(ChowLiu(sampling=t)(None).matrix, r.matrix)
        ptr, idx = r.structure()
        with Learner(t, structure=r.structure()) as L:
            tree_score = L.score()
            got_ptr, got_idx = L.structure()
        assert np.array_equal(got_ptr, ptr) and np.array_equal(got_idx, idx)
        with Learner(t) as L:
            assert tree_score < L.score()                                        # the chain explains the table better than no edges
        assert structure_model(k, ptr, idx).n == n


def test_tan(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import TAN, Learner
    n = 20
    pats, counts, k = chain_table(n, 4000, 3, seed=8, class_col=True)
    with InfoTable(pats, counts, k, device=0) as t:
        r = TAN(0)(t)
        check_tree(r, t.cond_pair_entropies(0)["cmi"])
        assert r.root == 1 and r.cond == 0 and t.info("tree_ns") > 0 and t.info("cond_pairs_ns") > 0
        assert np.array_equal(r.parent, [-1] + list(range(1, n - 1)))            # the chain over the features
        par = r.parents()
        assert par[0] == [] and par[1] == [0] and all(par[v] == [0, v - 1] for v in range(2, n))
        with Learner(t, structure=r.structure()) as L:
            assert np.isfinite(L.score())
        last = TAN(n - 1, root=5)(t, [7, 5, 6, 2])                               # another class, a subset, a given root
        check_tree(last, t.cond_pair_entropies(n - 1, [7, 5, 6, 2])["cmi"])
        assert last.root == 5 and all(n - 1 in last.parents()[v] for v in (7, 5, 6, 2)) and last.parents()[0] == []


def test_learner_refusals(bnlib):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import TAN, ChowLiu
    pats, counts, k = chain_table(6, 200, 3, seed=9)
    with InfoTable(pats, counts, k, device=0) as t:
        with pytest.raises(_lib.BnError, match="duplicate"):
            ChowLiu()(t, [0, 1, 1, 2])
        with pytest.raises(_lib.BnError, match="class"):
            TAN(2)(t, [0, 1, 2])
        with pytest.raises(_lib.BnError, match="root"):
            ChowLiu(root=5)(t, [0, 1, 2])
        with pytest.raises(_lib.BnError, match="range"):
            ChowLiu()(t, [0, 6])
        with pytest.raises(_lib.BnError, match="range"):
            TAN(6)(t)
        with pytest.raises(ValueError):
            ChowLiu()(None)
        one = ChowLiu()(t, [4])
        assert one.parent.tolist() == [-1] and one.weight.tolist() == [0.0] and one.parents()[4] == []
        assert ChowLiu()(t).parent[0] == -1                                      # the table still works


def test_sampler_route(bnlib):
    """A model with sampling=Sampler: the learners and the conditional matrix marshal the sampler's table for the call and give the
    InfoTable route's bits."""
    from types import SimpleNamespace
    from bayesiannetwork_amd.engine import Sampler
    from bayesiannetwork_amd.evaluation import InfoTable, conditional_mutual_information_matrix
    from bayesiannetwork_amd.learning import TAN, ChowLiu
    n = 8
    pats, _, k = chain_table(n, 500, 3, seed=10, class_col=True)
    rows, cnt = np.unique(pats, axis=0, return_counts=True)
    smp = Sampler()
    smp.load_sample({tuple(int(v) for v in row): int(c) for row, c in zip(rows, cnt)})
    model = SimpleNamespace(n=n, k=k)
    with InfoTable(rows, cnt.astype(np.uint64), k, device=0) as t:
        for mine, want in ((ChowLiu(sampling=smp)(model), ChowLiu()(t)), (TAN(0, sampling=smp)(model), TAN(0)(t)),
                           (TAN(3, sampling=smp, root=5)(model, [5, 1, 6]), TAN(3, root=5)(t, [5, 1, 6]))):
            assert np.array_equal(mine.parent, want.parent) and mine.root == want.root and mine.parents() == want.parents()
            assert same_bits(mine.matrix, want.matrix) and same_bits(mine.weight, want.weight)
        got = conditional_mutual_information_matrix(smp, 0, k=k)
        want = t.cond_pair_entropies(0)
        assert got["hz"] == want["hz"] and all(same_bits(got[key], want[key]) for key in ("hxz", "hxyz", "cmi"))
        got = conditional_mutual_information_matrix(smp, 4, [6, 2, 2], k=k)      # another order, a duplicate
        want = t.cond_pair_entropies(4, [6, 2, 2])
        assert all(same_bits(got[key], want[key]) for key in ("hxz", "hxyz", "cmi"))
        with pytest.raises(ValueError):
            conditional_mutual_information_matrix(smp, 2, [1, 2])
    empty = conditional_mutual_information_matrix(Sampler(), 0, [1, 2])
    assert empty["hz"] == 0.0 and not empty["cmi"].any() and empty["cmi"].shape == (2, 2)
