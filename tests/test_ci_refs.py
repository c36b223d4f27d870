"""The host restatement of the conditional-independence test (tests/ci_refs.py) against what does not depend on it: the chi-square
tail against 50-digit golden values (tests/golden/chisq_sf.json, made once by scripts/make_chisq_golden.py), and G, both
degrees-of-freedom rules and the marginals against a plain per-stratum computation on tiny tables."""
import json
import math
import os

import numpy as np
import pytest

import ci_refs as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_rows():
    with open(os.path.join(ROOT, "tests", "golden", "chisq_sf.json")) as f:
        return [(r["df"], float.fromhex(r["g"]), float(r["sf"])) for r in json.load(f)["rows"]]


def test_golden_grid_is_the_stated_grid():
    rows = golden_rows()
    assert [(df, g) for df, g, _ in rows] == C.golden_grid()
    # points on both sides of the series / fraction switch x < a + 1, i.e. G < df + 2
    assert any(g < df + 2.0 and 0.0 < sf < 1.0 for df, g, sf in rows) and any(g >= df + 2.0 and sf >= C.CHISQ_NORMAL for df, g, sf in rows)


def test_chisq_sf_against_golden_values():
    worst = 0.0
    for df, g, want in golden_rows():
        got = C.chisq_sf(g, df)
        assert not math.isnan(got) and 0.0 <= got <= 1.0
        if want >= C.CHISQ_NORMAL:
            worst = max(worst, abs(got - want) / want)
        assert C.tail_close(got, want), (df, g, got, want)
    print(f"worst relative error of the restatement over the grid: {worst:.3e} (recorded: {C.CHISQ_MEASURED:.3e})")
    assert worst <= C.CHISQ_MEASURED * 1.01   # the recorded figure is the measured one


def test_chisq_sf_edges():
    assert C.chisq_sf(0.0, 5) == 1.0 and C.chisq_sf(3.0, 0) == 1.0 and C.chisq_sf(-0.0, 1) == 1.0
    assert C.chisq_sf(1e6, 3) == 0.0                       # a vanished tail
    assert 0.0 < C.chisq_sf(1420.0, 2) < 1e-300            # exp(-710): a denormal or nearly
    assert C.chisq_sf(2.0, 2) == pytest.approx(math.exp(-1.0), rel=1e-15)   # df = 2: the tail is exp(-G / 2)
    ladder = [C.chisq_sf(g, 7) for g in (0.5, 1.0, 2.0, 7.0, 8.9, 9.1, 20.0, 200.0)]
    assert all(a > b for a, b in zip(ladder, ladder[1:]))


def plain(N):
    """G, nominal df, adjusted df stratum by stratum with numpy."""
    N = np.asarray(N, dtype=np.float64)
    g, adf = 0.0, 0
    for T in N:
        tot, r, c = T.sum(), T.sum(axis=1), T.sum(axis=0)
        if tot == 0:
            continue
        E = np.outer(r, c) / tot
        nz = T > 0
        g += 2.0 * float((T[nz] * np.log(T[nz] / E[nz])).sum())
        adf += (int((r > 0).sum()) - 1) * (int((c > 0).sum()) - 1)
    return g, (N.shape[1] - 1) * (N.shape[2] - 1) * N.shape[0], adf


@pytest.mark.parametrize("seed, k, x, y, S", [(1, [3, 2, 2, 4], 0, 3, [1, 2]), (2, [2, 5, 3], 1, 0, []), (3, [4, 3, 2, 2, 3], 4, 1, [3, 0, 2])])
def test_g_df_and_marginals_from_first_principles(seed, k, x, y, S):
    rng = np.random.default_rng(seed)
    pats = np.stack([rng.integers(0, kk, 40) for kk in k], axis=1).astype(np.uint8)
    w = rng.integers(1, 9, 40).astype(np.uint64)
    g, df, p, N = C.run_test(pats, w, k, x, y, S)
    assert N.shape == (math.prod(k[v] for v in S), k[y], k[x]) and int(N.sum()) == int(w.sum())
    brute = np.zeros(N.shape, dtype=np.uint64)   # cell by cell, S sorted, first most significant
    for row, c in zip(pats, w):
        s = 0
        for u in sorted(S):
            s = s * k[u] + int(row[u])
        brute[s, row[y], row[x]] += c
    assert np.array_equal(N, brute)
    Ns, R, Cc = C.marginals(N)
    assert all(int(Ns[s]) == int(N[s].sum()) for s in range(N.shape[0]))
    assert np.array_equal(R.astype(np.uint64), N.sum(axis=2)) and np.array_equal(Cc.astype(np.uint64), N.sum(axis=1))
    want_g, want_df, want_adf = plain(N)
    assert g == pytest.approx(want_g, rel=1e-12) and df == want_df == C.df_nominal(N) and C.df_adjusted(N) == want_adf
    assert abs(g - C.g_exact(N)) <= C.g_bound(N)
    assert p == C.chisq_sf(g, df)


def test_adjusted_df_on_empty_and_degenerate_strata():
    N = np.zeros((3, 2, 3), dtype=np.uint64)
    N[0] = [[4, 1, 2], [3, 5, 1]]          # full: (2 - 1) * (3 - 1)
    N[2, 1] = [7, 0, 2]                    # one non-zero row: 0; stratum 1 is empty: 0
    assert C.df_adjusted(N) == 2 and C.df_nominal(N) == 6
    assert C.g2(N) == C.g2(N[:1])          # the degenerate strata add exactly nothing
    one = np.array([[[5], [7]]], dtype=np.uint64)   # an arity-1 x
    assert C.g2(one) == 0.0 and C.df_nominal(one) == 0 and C.chisq_sf(0.0, 0) == 1.0
