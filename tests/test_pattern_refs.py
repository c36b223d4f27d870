"""The host references of tests/pattern_refs.py pinned without a GPU: the limb-split one-hot GEMM against np.add.at
(counts near 2^63, zero counts, a tiled table), the decimal entropy against hand values and against np_entropy,
the long-double all-pairs form against the decimal one, and the numpy CPT fit against the C restatement."""
import math

import numpy as np
import pytest

from pattern_refs import (block, cell_counts, cpt_edge_model, entropy_bound, entropy_exact, entropy_ld, fit_cpt_ref,
                          pair_count_matrix, pair_entropies_ref, random_patterns, tiled_pair_count_matrix, tiled_table)
from test_entropy_host import np_entropy


def add_at_block(pats, counts, x, y, kx, ky):
    out = np.zeros(kx * ky, np.uint64)
    np.add.at(out, pats[:, x].astype(np.int64) * ky + pats[:, y], np.asarray(counts, np.uint64))
    return out.reshape(kx, ky)


def big_counts(r, P):
    """Counts with zeros, small values and a few near 2^63, the total still below 2^64."""
    c = r.integers(0, 1 << 20, P).astype(np.uint64)
    c[r.random(P) < 0.2] = 0
    c[3] = np.uint64((1 << 63) - 12345)
    c[P // 2] = np.uint64(1 << 61)
    c[P - 1] = np.uint64((1 << 62) + 1)
    return c


@pytest.mark.parametrize("kind", ["one", "big"])
def test_pair_count_matrix_equals_add_at(kind):
    r = np.random.default_rng(1)
    k = np.array([1, 2, 3, 4, 7, 16, 33, 255], np.int32)
    P = 700
    pats = random_patterns(k, P, 2)
    c = np.ones(P, np.uint64) if kind == "one" else big_counts(r, P)
    assert int(c.astype(object).sum()) < 1 << 64
    M = pair_count_matrix(pats, c, k)
    for x in range(len(k)):
        for y in range(len(k)):
            assert np.array_equal(block(M, k, x, y), add_at_block(pats, c, x, y, k[x], k[y])), (x, y)
    assert np.array_equal(M, M.T)


def test_tiled_reference_equals_the_full_table():
    k = np.array([2, 5, 3], np.int32)
    base = random_patterns(k, 37, 3)
    bc = np.random.default_rng(4).integers(0, 1000, 37).astype(np.uint64)
    pats, c = tiled_table(base, bc, 9, 11)
    assert len(c) == 37 * 9 + 11
    assert np.array_equal(tiled_pair_count_matrix(base, bc, k, 9, 11), pair_count_matrix(pats, c, k))
    assert np.array_equal(tiled_pair_count_matrix(base, bc, k, 9, 0), pair_count_matrix(*tiled_table(base, bc, 9, 0), k))


def test_entropy_exact_hand_values():
    for j in range(0, 12):
        assert entropy_exact([3] * (1 << j)) == float(j)
    assert entropy_exact([1 << 62] * 4) == 2.0
    assert entropy_exact([(1 << 63) - 1]) == 0.0
    assert entropy_exact([0, 5, 0, 5, 0]) == 1.0          # zero cells add nothing
    assert entropy_exact([0, 0]) == 0.0
    assert entropy_exact([1, 3]) == pytest.approx(2 - 0.75 * math.log2(3), rel=1e-15)
    # one count against 2^63 - 1: H = -(1 - p) log2(1 - p) - p log2(p), p = 2^-63
    p = 2.0 ** -63
    want = -(1 - p) * math.log1p(-p) / math.log(2) + p * 63
    assert entropy_exact([(1 << 63) - 1, 1]) == pytest.approx(want, rel=1e-14)


def test_entropy_exact_agrees_with_np_entropy_and_bincount():
    r = np.random.default_rng(7)
    for trial in range(6):
        k = r.integers(1, 9, 4).astype(np.int32)
        pats = random_patterns(k, 500, trial)
        c = r.integers(1, 1 << 30, 500).astype(np.uint64)
        for cols in ([0], [1, 2], [0, 1, 2, 3], [3, 1]):
            cells = cell_counts(pats, c, cols)
            assert sum(cells) == int(c.astype(object).sum())
            key = np.zeros(500, np.int64)
            for col in sorted(cols):
                key = key * int(k[col]) + pats[:, col]
            # np.bincount's float64 sums are exact here (totals < 2^53)
            bc = np.bincount(key, c.astype(np.float64))
            assert sorted(cells) == sorted(int(x) for x in bc[bc > 0])
            H = entropy_exact(cells)
            assert abs(H - np_entropy(pats, c, cols)) <= entropy_bound(H, len(cells))


def test_entropy_ld_and_pair_reference_agree_with_decimal():
    r = np.random.default_rng(9)
    k = np.array([1, 2, 3, 4, 9, 17], np.int32)
    P = 400
    pats = random_patterns(k, P, 5)
    c = big_counts(r, P)
    N = int(c.astype(object).sum())
    M = pair_count_matrix(pats, c, k)
    hxy, nnz = pair_entropies_ref(M, k, N)
    for x in range(len(k)):
        for y in range(len(k)):
            b = block(M, k, x, y)
            exact = entropy_exact(b)
            assert nnz[x, y] == int((b > 0).sum())
            assert abs(hxy[x, y] - exact) <= 1e-3 * entropy_bound(exact, nnz[x, y]) or hxy[x, y] == exact, (x, y)
            assert exact == entropy_exact(cell_counts(pats, c, [x, y]))
    assert float(entropy_ld(np.array([[1 << 62] * 4], np.uint64), 1 << 64)[0]) == 2.0


def test_entropy_bound_is_tight_enough_to_see_a_lost_count():
    """One count moved between cells or dropped moves H by far more than the bound, at the sizes the GPU tests use."""
    r = np.random.default_rng(3)
    cells = [int(x) for x in r.integers(1, 1 << 40, 16)]
    H = entropy_exact(cells)
    moved = list(cells)
    moved[0] += 1 << 20
    moved[1] -= 1 << 20
    assert abs(entropy_exact(moved) - H) > 100 * entropy_bound(H, 16)
    unit = [1] * 3000
    H1 = entropy_exact(unit)
    assert abs(entropy_exact(unit[:-1]) - H1) > 100 * entropy_bound(H1, 3000)


@pytest.mark.parametrize("P", [1, 1000])
def test_fit_cpt_reference_equals_the_c_restatement(oracle_mod, P):
    m = cpt_edge_model()
    pats = random_patterns(m.k, P, 11)
    c = np.random.default_rng(12).integers(0, 1 << 20, P).astype(np.uint64)
    c[0] = np.uint64(1 << 62)
    assert np.array_equal(fit_cpt_ref(m, pats, c), oracle_mod.make_cpt(m, pats, c))
    assert int(np.diff(m.cpt_off).max()) == 1 << 17
    assert {4096, 4097, 65536, 65025} <= set(int(s) for s in np.diff(m.cpt_off))
