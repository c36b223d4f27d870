"""tests/tree_refs.py checked against brute force: Kruskal's tree under the library's edge order is the maximum-weight tree among all
n^(n - 2) labelled trees and the first of the maximal ones under that order; orientation from every root; the grouped decimal entropy
equals pattern_refs.entropy_exact; the conditional counts agree with pattern_refs.cell_counts.  No GPU."""
import numpy as np
import pytest

import pattern_refs as R
import tree_refs as TR


def matrices():
    rng = np.random.default_rng(5)
    out = []
    for n in range(1, 7):
        for _ in range(4):
            out.append(rng.integers(-50, 50, (n, n)).astype(np.float64))      # random: few ties
            out.append(rng.integers(0, 3, (n, n)).astype(np.float64))         # heavily tied
        out.append(np.full((n, n), 7.0))                                      # all equal
        z = rng.integers(0, 2, (n, n)).astype(np.float64)
        out.append(np.where(rng.random((n, n)) < 0.5, -0.0, 0.0) * (z + 1))   # -0.0 against 0.0: all equal under the order
    return out


def total(w, tree):
    return sum(w[a, b] for a, b in tree)


def order_key(w, tree):
    """A tree as the sequence of its edges sorted by the edge order: the first tree under the order has the smallest sequence."""
    return sorted(TR.edge_key(w[a, b], a, b) for a, b in tree)


@pytest.mark.parametrize("index", range(len(matrices())))
def test_kruskal_is_the_first_maximal_tree(index):
    w = matrices()[index]
    n = w.shape[0]
    mine = tuple(sorted(TR.kruskal_edges(w)))
    trees = list(TR.all_trees(n))
    assert len(trees) == (1 if n < 3 else n ** (n - 2)) and len(set(trees)) == len(trees)
    assert mine in trees
    best = max(total(w, t) for t in trees)
    assert total(w, mine) == best
    maximal = [t for t in trees if total(w, t) == best]
    assert order_key(w, mine) == min(order_key(w, t) for t in maximal)
    # the lower triangle is not read
    w2 = np.triu(w, 1) + np.tril(np.full((n, n), 1e9), -1)
    assert tuple(sorted(TR.kruskal_edges(w2))) == mine


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6])
def test_orientation_from_every_root(n):
    rng = np.random.default_rng(n)
    w = rng.integers(0, 4, (n, n)).astype(np.float64)
    edges = set(TR.kruskal_edges(w))
    for root in range(n):
        parent = TR.kruskal(w, root)
        assert parent[root] == -1 and (np.delete(parent, root) >= 0).all()      # one parent each, every node reached
        assert {(min(v, int(p)), max(v, int(p))) for v, p in enumerate(parent) if p >= 0} == edges
        for v in range(n):                                                      # every node's path ends at the root
            steps = 0
            while parent[v] >= 0:
                v, steps = int(parent[v]), steps + 1
                assert steps < n
            assert v == root


def test_grouped_entropy_and_conditional_counts():
    rng = np.random.default_rng(2)
    for cells in ([1], [5, 5, 5, 1], rng.integers(0, 6, 200), rng.integers(1, 1 << 40, 50), [128] * 37 + [256] * 5):
        assert TR.entropy_exact_grouped(cells) == R.entropy_exact(cells)
        assert float(TR.entropy_exact_grouped(cells, rounded=False)) == R.entropy_exact(cells)
    k = np.array([3, 4, 2, 5])
    pats = np.stack([rng.integers(0, kk, 300) for kk in k], axis=1).astype(np.uint8)
    counts = rng.integers(0, 1 << 41, 300).astype(np.uint64)
    for x, y, z in [(0, 1, 2), (1, 0, 3), (3, 3, 0)]:
        c = TR.cond_counts(pats, counts, k, x, y, z)
        assert int(c.sum(dtype=np.uint64)) == int(counts.sum(dtype=np.uint64))
        assert sorted(int(v) for v in c.ravel() if v) == sorted(R.cell_counts(pats, counts, [x, y, z]))
        key = (pats[:, z].astype(np.int64) * int(k[x]) + pats[:, x]) * int(k[y]) + pats[:, y]
        assert sorted(int(v) for v in TR.cells_by_key(key, counts)) == sorted(int(v) for v in c.ravel() if v)
        assert np.array_equal(c, TR.cond_counts(pats, counts, k, y, x, z).transpose(0, 2, 1))
    assert TR.cond_entropy_bound(1.0, 10, 4) == R.entropy_bound(1.0, 14)
