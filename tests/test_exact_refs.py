"""The exact references of tests/exact_refs.py, and the C restatement of the reference (oracle/bp_oracle.c) against them.

The golden fixtures tie the oracle to the reference on networks of at most 4 parents, arities 2-4 and 1 000 nodes; these
tests tie it to exact inference beyond that: 16 parents, arities 1-255, zero CPT entries, chains thousands of nodes deep
and 20 000-node forests.  Every comparison runs a fixed number of sweeps (eps = 0, max_sweeps = sweeps_needed): the
reference's stopping rule can end a run before the answer is exact (test_early_stop_is_the_reference_rule).

Measured maximum |oracle - exact| over these families: 1.6e-15 (wide16); 2.2e-16 or less elsewhere."""
import numpy as np
import pytest

import exact_refs as X
import oracle

DBL_MIN = np.finfo(np.float64).tiny
TOL = 1e-14


FAMILIES = X.families()


def test_two_pass_equals_rational_enumeration():
    """>= 20 tiny polytrees, hard / soft / mixed evidence, some with zero CPT entries: the long-double two-pass result equals
    exact rational enumeration of the same split model to 1e-15."""
    worst, moved = 0.0, 0
    for s in range(24):
        m = X.polytree(6, (2, 3), max_parents=3, max_children=3, zero_frac=0.2 if s % 3 == 0 else 0.0, seed=s)
        ev = X.draw_evidence(m, 2, seed=100 + s, soft=(0.0, 1.0, 0.5)[s % 3])
        got, _ = X.exact_marginals(m, ev)
        want = np.concatenate([[float(x) for x in row] for row in X.brute_force_marginals(m, ev)])
        worst = max(worst, float(np.abs(got - want).max()))
        moved += not np.allclose(got, X.exact_marginals(m, None)[0], atol=1e-6)
    assert worst <= 1e-15, worst
    assert moved >= 20, "the evidence should move the marginals"


def test_einsum_elimination_equals_two_pass():
    """On polytrees the two exact references agree (hard evidence, unnormalised joints P(x_v = s, e))."""
    for s in range(6):
        m = X.polytree(12, (2, 3, 4), 3, 3, zero_frac=0.2 * (s % 2), seed=40 + s)
        st = np.full(m.n, -1, dtype=np.int32)
        ev = X.draw_evidence(m, 3, seed=s)
        st[ev.node] = ev.hard_states(m)[ev.node]
        a = X.exact_joint(m, st)
        b, pe = X.einsum_marginals(m, st)
        assert 0 < pe <= 1 and np.abs(a - b).max() <= 1e-15


def test_sweeps_needed():
    assert X.sweeps_needed(X.chain(10)) == 2 * 9 + 4
    assert X.sweeps_needed(X.wide(5)) == 2 * 2 + 4
    assert X.sweeps_needed(X.disjoint_union([X.chain(3), X.chain(7)])) == 2 * 6 + 4


def test_the_generators_keep_their_promises():
    f = dict((n, m) for n, m, _ in FAMILIES)
    assert int(np.diff(f["wide16"].in_ptr).max()) == 16
    assert {1, 2, 5, 7, 9, 17, 255} <= set(f["arity255"].k.tolist())
    k255 = f["arity255"]
    assert any(k255.k[v] == 255 and any(k255.k[p] == 255 for p in k255.parents(v)) for v in range(k255.n))
    z = f["zeros"]
    assert 0.15 < float((z.cpt == 0).mean()) < 0.35 and all((z.cpt_of(v) > 0).any(axis=1).all() for v in range(z.n))
    assert f["deep"].n >= 3000 and X.sweeps_needed(f["deep"]) >= 6000
    fo = f["forest"]
    ch = np.bincount(fo.in_idx, minlength=fo.n)
    assert fo.n == 20000 and int(np.diff(fo.in_ptr).max()) == 2 and int(ch.max()) <= 8
    assert int(np.diff(f["dagmix"].in_ptr).max()) == 5 and set(f["dagmix"].k.tolist()) == {2, 3, 4}
    assert int(np.bincount(f["hub"].in_idx).max()) == 1000


@pytest.mark.parametrize("name", [n for n, _, _ in FAMILIES])
def test_oracle_equals_exact_at_pinned_sweeps(oracle_mod, name):
    """oracle.bp_run(eps = 0, max_sweeps = S) equals the exact marginals on every family, with and without evidence."""
    _, m, evs = next(f for f in FAMILIES if f[0] == name)
    S = X.sweeps_needed(m)
    for ev in [None] + evs:
        want, _ = X.exact_marginals(m, ev)
        got = oracle_mod.bp_run(m, ev, eps=0.0, max_sweeps=S, threads=8, res_cap=S)
        assert got["sweeps"] == S
        assert np.abs(got["beliefs"] - want).max() <= TOL, (name, float(np.abs(got["beliefs"] - want).max()))


def test_early_stop_is_the_reference_rule(oracle_mod):
    """Regression fixture for the stopping rule: on this 7-node polytree with two soft-evidence nodes the run stops at sweep 5,
    a sweep that changed no message (residual DBL_MIN), while the news is still in the node vectors: a belief is > 1e-3
    from exact.  Pinned to S sweeps it is exact, and its residual history still holds DBL_MIN entries (sweeps 5 and 7)."""
    m, ev = X.early_stop_case()
    want, _ = X.exact_marginals(m, ev)
    r = oracle_mod.bp_run(m, ev, eps=1e-13)
    assert r["sweeps"] == 5 and r["residuals"][-1] == DBL_MIN
    assert np.abs(r["beliefs"] - want).max() > 1e-3
    S = X.sweeps_needed(m)
    r = oracle_mod.bp_run(m, ev, eps=0.0, max_sweeps=S)
    assert r["sweeps"] == S and r["residuals"][5] > 1e-3 and (r["residuals"] == DBL_MIN).sum() >= 2
    assert np.abs(r["beliefs"] - want).max() <= TOL


SMALL_FOR_REF = ["wide5", "wide8", "wide9", "arity17", "star", "zeros"]


@pytest.mark.skipif(not oracle.ref_available(), reason="oracle/_ref/ref_driver is not built here (it needs the reference sources)")
@pytest.mark.parametrize("name", SMALL_FOR_REF)
def test_reference_equals_exact_on_small_families(oracle_mod, name):
    """The reference itself against the exact split model, so the soft-evidence clamp is pinned to the reference and not only
    to its restatement.  The reference has no sweep cap, so it runs with eps = 1e-300 and stops where a sweep changes no
    message; on these networks that happens after the news has arrived (measured: within 2.2e-16 of exact)."""
    _, m, evs = next(f for f in FAMILIES if f[0] == name)
    for ev in evs:
        r = oracle_mod.ref_bp(m, ev, eps=1e-300, timeout=600)
        if int(np.diff(m.in_ptr).max()) <= 2:   # (with >= 3 parents the reference multiplies in unordered_map order)
            assert r["sweeps"] == oracle_mod.bp_run(m, ev, eps=1e-300)["sweeps"]
        got = np.concatenate([np.asarray(b, dtype=np.float64).ravel() for b in r["beliefs"]])
        want, _ = X.exact_marginals(m, ev)
        assert np.abs(got - want).max() <= TOL


@pytest.mark.skipif(not oracle.ref_available(), reason="oracle/_ref/ref_driver is not built here (it needs the reference sources)")
def test_reference_stops_early_like_the_oracle(oracle_mod):
    m, ev = X.early_stop_case()
    r = oracle_mod.ref_bp(m, ev, eps=1e-13)
    o = oracle_mod.bp_run(m, ev, eps=1e-13)
    assert r["sweeps"] == o["sweeps"] == 5 and np.array_equal(np.asarray(r["residuals"]), o["residuals"])
    got = np.concatenate([np.asarray(b, dtype=np.float64).ravel() for b in r["beliefs"]])
    assert np.array_equal(got, o["beliefs"])
