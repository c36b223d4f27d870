"""bn_ci_tests and bn_ci_chisq_sf on the device against the host restatement (tests/ci_refs.py): exact counts, both degrees-of-freedom
rules, G within the derived bound, the tail within the measured tolerance, at the smallest shapes where the kernel takes another
path; the same bits for a test wherever it stands; and the refusals, with nothing launched."""
import json
import math
import os

import numpy as np
import pytest

import ci_refs as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# columns:  0    1   2   3  4   5   6  7  8   9  10  11 .. 20
K = [3, 5, 17, 4, 4, 16, 16, 2, 3, 43, 1] + [2] * 10
P_ROWS = 700
# name: (x, y, S): the cells k_x * k_y * prod k_S on either side of the 256 partial sums, and of the 4096 cells up to which the
# counters are kept in LDS; |S| = 0 and 8; an arity-1 x; y's id below, between and above S's ids
TESTS = {
    "cells255": (0, 1, [2]), "cells256": (3, 4, [5]), "cells258": (7, 8, [9]), "cells4096": (3, 4, [6, 5]), "cells4352": (3, 4, [6, 2]),
    "s0": (0, 1, []), "s8": (11, 12, [20, 13, 19, 14, 18, 15, 17, 16]), "arity1": (10, 1, [7]),
    "y_below": (3, 0, [5, 6]), "y_between": (7, 5, [9, 2]), "y_above": (0, 20, [1, 2]),
}
_REF = {}


def table_data():
    if "data" not in _REF:
        rng = np.random.default_rng(77)
        pats = np.stack([rng.integers(0, kk, P_ROWS) for kk in K], axis=1).astype(np.uint8)
        pats[:, 4] = np.where(rng.random(P_ROWS) < 0.7, pats[:, 3], pats[:, 4])     # column 4 depends on column 3
        pats[:, 12] = np.where(rng.random(P_ROWS) < 0.6, pats[:, 11], pats[:, 12])
        w = rng.integers(1, 6, P_ROWS).astype(np.uint64)
        _REF["data"] = (pats, w)
    return _REF["data"]


def ref(name, rule):
    """(N, G by libm in the stated order, df) of a named test; computed once."""
    if (name, rule) not in _REF:
        pats, w = table_data()
        x, y, S = TESTS[name]
        N = C.counts(pats, w, K, x, y, S)
        _REF[(name, rule)] = (N, C.g2(N), C.df_of(N, rule))
    return _REF[(name, rule)]


@pytest.fixture(scope="module")
def table(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    pats, w = table_data()
    with InfoTable(pats, w, K, device=0) as t:
        yield t


def check(out, i, N, rule):
    g, df, p = float(out["stat"][i]), int(out["df"][i]), float(out["p"][i])
    bound = C.g_bound(N)
    print(f"  G {g!r} libm {C.g2(N)!r} |G - exact| {abs(g - C.g_exact(N)):.3e} bound {bound:.3e}; df {df}; p {p!r} "
          f"restated {C.chisq_sf(g, df)!r}")
    assert df == C.df_of(N, rule)
    assert g >= 0.0 and abs(g - C.g_exact(N)) <= bound
    assert not math.isnan(p) and C.tail_close(p, C.chisq_sf(g, df))
    assert bool(out["independent"][i]) == (p > 0.05)


@pytest.mark.parametrize("rule", ["nominal", "adjusted"])
def test_counts_df_statistic_and_tail(table, rule):
    from bayesiannetwork_amd.evaluation import ci_tests
    names = list(TESTS)
    assert [math.prod(K[v] for v in (x, y) + tuple(S)) for x, y, S in (TESTS[n] for n in names[:5])] == [255, 256, 258, 4096, 4352]
    out = ci_tests(table, [TESTS[n] for n in names], df_rule=rule, counts=True)
    for i, name in enumerate(names):
        N, _, df = ref(name, rule)
        print(name, TESTS[name])
        assert out["counts"][i].shape == N.shape and np.array_equal(out["counts"][i], N)      # exact
        check(out, i, N, rule)
    N = ref("arity1", rule)[0]
    i = names.index("arity1")
    assert out["stat"][i] == 0.0 and out["df"][i] == 0 and out["p"][i] == 1.0
    # the table has what the adjusted rule is about: an empty stratum, and a stratum with one non-zero row
    Ns, R, _ = C.marginals(ref("cells4352", "adjusted")[0])
    assert any(v == 0 for v in Ns) and any(Ns[s] != 0 and np.count_nonzero(R[s]) == 1 for s in range(len(Ns)))
    assert ref("cells4352", "adjusted")[2] < ref("cells4352", "nominal")[2]


def test_weight_above_2_32(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable, ci_tests
    pats, w = table_data()
    pats, w = pats[:60], w[:60].copy()
    w[5], w[17] = (1 << 33) + 5, (1 << 32) + 1
    with InfoTable(pats, w, K, device=0) as t:
        out = ci_tests(t, [TESTS["cells255"], TESTS["cells4352"]], df_rule="adjusted", counts=True)
    for i, name in enumerate(("cells255", "cells4352")):
        N = C.counts(pats, w, K, *TESTS[name])
        assert int(N.max()) > (1 << 33) and np.array_equal(out["counts"][i], N)
        check(out, i, N, "adjusted")


def test_one_pattern_table(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable, ci_tests
    with InfoTable(np.array([[1, 0, 2]], dtype=np.uint8), np.array([9], dtype=np.uint64), [2, 2, 3], device=0) as t:
        out = ci_tests(t, [(0, 1, [2]), (0, 1, [])], df_rule="adjusted", counts=True)
    assert out["stat"].tolist() == [0.0, 0.0] and out["df"].tolist() == [0, 0] and out["p"].tolist() == [1.0, 1.0]
    assert int(out["counts"][0].sum()) == 9 and out["counts"][0][2, 0, 1] == 9


def bits(out, i):
    return (float(out["stat"][i]).hex(), int(out["df"][i]), float(out["p"][i]).hex())


def test_same_bits_wherever_a_test_stands(table, bnlib, monkeypatch):
    from bayesiannetwork_amd.evaluation import InfoTable, ci_tests
    a, b, c = TESTS["cells255"], TESTS["cells256"], TESTS["cells258"]
    alone = ci_tests(table, [a])
    twice = ci_tests(table, [a, b, (a[0], a[1], list(reversed(a[2]))), c, TESTS["cells4352"]])
    assert bits(alone, 0) == bits(twice, 0) == bits(twice, 2)
    before = table.info("ci_launches")
    monkeypatch.setenv("BN_CI_SCRATCH_CELLS", "400")     # the three groups hold 306, 320 and 344 cells: three passes
    passes = ci_tests(table, [c, b, a])
    monkeypatch.delenv("BN_CI_SCRATCH_CELLS")
    assert table.info("ci_launches") - before == 6        # a counting and a statistic launch per pass
    assert bits(passes, 2) == bits(alone, 0) and bits(passes, 1) == bits(twice, 1) and bits(passes, 0) == bits(twice, 3)
    pats, w = table_data()
    perm = np.random.default_rng(3).permutation(P_ROWS)
    with InfoTable(pats[perm], w[perm], K, device=0) as shuffled:
        again = ci_tests(shuffled, [b, a, TESTS["cells4352"]])
    assert bits(again, 1) == bits(alone, 0) and bits(again, 0) == bits(twice, 1) and bits(again, 2) == bits(twice, 4)


def golden_rows():
    with open(os.path.join(ROOT, "tests", "golden", "chisq_sf.json")) as f:
        return [(r["df"], float.fromhex(r["g"]), float(r["sf"])) for r in json.load(f)["rows"]]


def test_chisq_sf_on_the_device(bnlib):
    from bayesiannetwork_amd.evaluation import chisq_sf
    rows = golden_rows()
    got = chisq_sf([g for _, g, _ in rows], [df for df, _, _ in rows])
    worst = 0.0
    for (df, g, want), p in zip(rows, got.tolist()):
        if want >= C.CHISQ_NORMAL:
            worst = max(worst, abs(p - want) / want)
    print(f"worst relative error of the device over the grid: {worst:.3e} (tolerance {C.CHISQ_TOL:.3e})")
    for (df, g, want), p in zip(rows, got.tolist()):
        assert not math.isnan(p) and 0.0 <= p <= 1.0
        assert C.tail_close(p, want), (df, g, p, want)
    for df in (1, 7, 64):   # monotone in G on a short ladder across the series / fraction switch
        ladder = sorted({0.25 * df, 0.5 * df, float(df), df + 1.9, df + 2.1, 2.0 * df + 3.0, 4.0 * df + 4.0})
        ps = chisq_sf(ladder, [df] * len(ladder)).tolist()
        assert all(x > y for x, y in zip(ps, ps[1:])), (df, ps)


@pytest.mark.parametrize("bad, cause", [
    ((3, 3, []), "same variable"), ((3, 4, [5, 3]), "is in the conditioning set"), ((3, 4, [5, 6, 5]), "listed twice"),
    ((11, 12, [13, 14, 15, 16, 17, 18, 19, 20, 7]), "9 variables"), ((5, 6, [2, 9, 3, 4]), "cells"),
])
def test_refusals_launch_nothing(table, bnlib, bad, cause):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.evaluation import ci_tests
    before = table.info("ci_launches")
    with pytest.raises(_lib.BnError) as e:
        ci_tests(table, [TESTS["s0"], bad])
    assert e.value.code == _lib.BN_ERR_ARG and "test 1" in str(e.value) and cause in str(e.value)
    assert table.info("ci_launches") == before and table.info("ci_stat_ns") == 0 and table.info("ci_count_ns") == 0


@pytest.mark.parametrize("alpha", [0.0, 1.0, -0.5, float("nan")])
def test_alpha_outside_the_open_interval_is_refused(table, bnlib, alpha):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.evaluation import ci_tests
    before = table.info("ci_launches")
    with pytest.raises(_lib.BnError) as e:
        ci_tests(table, [TESTS["s0"]], alpha=alpha)
    assert e.value.code == _lib.BN_ERR_ARG and "alpha" in str(e.value) and table.info("ci_launches") == before
