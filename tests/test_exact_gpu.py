"""Every BP path, and the samplers, against EXACT inference (tests/exact_refs.py) instead of against the C restatement.

Each BP case forces its path and asserts it ran (last_path, the layout's tile variants, info(...)), runs a fixed number
of sweeps (eps = 0, max_sweeps = S = sweeps_needed: the reference's stopping rule can end a run early, see
test_exact_refs.py) and asserts the sweep count and beliefs within 1e-12 absolute of the exact marginals (every path
met that bound on an MI355X; the oracle itself is within 1.6e-15).

Likelihood weighting with hard evidence: every weight is in [0, 1], so the variance of w 1{x_v = s} is at most its mean
P(x_v = s, e) and |hist / n - P(x_v = s, e)| <= 6 sqrt(P / n) + 1e-12 (exact joints from the two-pass reference on polytrees,
np.einsum elimination on loopy networks).  Rejection sampling: a binomial 6-sigma band around the exact posterior.
test_lw_equals_exact_joint[arity255] found the generic kernel giving one-state nodes other states (see bn_lw_kernels.hip,
pick_states16); arity17_k1 keeps that case at a smaller size."""
import functools

import numpy as np
import pytest

import exact_refs as X
import oracle
from bayesiannetwork_amd import Evidence, from_parent_lists

pytestmark = pytest.mark.gpu

TOL = 1e-12
DBL_MIN = np.finfo(np.float64).tiny


@pytest.fixture(scope="module")
def Engine(bnlib):
    from bayesiannetwork_amd.engine import Engine
    return Engine


@functools.lru_cache(maxsize=None)
def fam(name):
    for n, m, evs in X.families():
        if n == name:
            return m, evs
    extra = {
        "group4": lambda: X.polytree(600, (4,), 5, 6, seed=8, name="group4"),           # k = 4, 3-5 parents: lane-group tiles
        "forest14k": lambda: X.forest(14000, 4, 2, 8, seed=4),                           # within the item kernels' 60 000 entries
        "big": lambda: X.forest(100000, 4, 4, 8, seed=9, tree_size=5000),               # the DAG path's stream form
    }
    m = extra[name]()
    return m, [X.draw_evidence(m, max(4, m.n // 100), seed=11, soft=0.3)]


@functools.lru_cache(maxsize=None)
def exact(name, i):
    m, evs = fam(name)
    return X.exact_marginals(m, evs[i])[0]


def variants(eng):
    return {c["variant"] for c in eng.layout_classes()}


def force(eng, path, flow=0):
    if path == 0:
        eng.set_option("multisweep", 0)
    elif path == 2:
        for o in ("small", "mid", "dag"):
            eng.set_option(o, 0)
        eng.set_option("multisweep", 2)
        eng.set_option("flow", flow)
    elif path == 3:
        eng.set_option("dag", 0)
        eng.set_option("small", 2)
    elif path == 4:
        eng.set_option("dag", 0)
        eng.set_option("small", 0)
        eng.set_option("mid", 2)
    elif path == 5:
        eng.set_option("dag", 2)
        eng.set_option("dagflow", flow)


def assert_ran(eng, path, flow=0):
    assert eng.last_path() == path
    if path == 2:
        assert eng.info("last_flow") == flow
    if path == 5:
        assert eng.info("last_dag_flow") == flow and eng.info("dag_aborts") == 0


# one evidence set only: the one-lane generic tile walks wide16's 65 536-row table and arity255's 255 x 255 table serially
# (measured: about 7 s per sweep on wide16, 0.8 s on arity255)
SLOW = {"wide16", "arity255"}


def check_exact(eng, name, path, flow=0, view=False):
    m, evs = fam(name)
    evs = evs[:1] if name in SLOW else evs
    S = X.sweeps_needed(m)
    worst = 0.0
    for i, ev in enumerate(evs):
        r = (eng.bp_run_view if view else eng.bp_run)(ev, 0.0, S)
        assert_ran(eng, path, flow)
        assert r["sweeps"] == S
        worst = max(worst, float(np.abs(r["beliefs"] - exact(name, i)).max()))
    assert worst <= TOL, (name, path, worst)
    return worst


# ---- one launch per sweep (path 0): every tile variant ---------------------------------------

LAUNCH = [  # family, lanes_per_node, tile variant that must be in the layout
    ("forest", 0, 1), ("deep", 0, 1), ("group4", 0, 2),
    ("wide5", 0, 3), ("wide8", 0, 3), ("arity17", 0, 3), ("star", 0, 3), ("zeros", 0, 3), ("hub", 0, 3),
    ("wide9", 0, 0), ("wide12", 0, 0), ("wide16", 0, 0), ("arity255", 0, 0),
    ("arity17", 1, 0), ("dagmix", 1, 0), ("wide8", 1, 0),
]


@pytest.mark.parametrize("name,lanes,variant", LAUNCH, ids=[f"{n}-lpn{lp}-v{v}" for n, lp, v in LAUNCH])
def test_launch_path_equals_exact(Engine, name, lanes, variant):
    m, _ = fam(name)
    with Engine(m, lanes_per_node=lanes) as eng:
        assert variant in variants(eng)
        if lanes == 1:
            assert variants(eng) <= {0, 1}
        force(eng, 0)
        check_exact(eng, name, 0)


# ---- the one-launch paths ----------------------------------------------------------------------

@pytest.mark.parametrize("name,flow", [("forest", 0), ("forest", 1), ("deep", 0), ("forest14k", 1)])
def test_resident_equals_exact(Engine, name, flow):
    """Resident tiles (uniform tiles only: lanes_per_node = 1 keeps the forest's many-children nodes off the any-arity
    tiles), flow 0 and 1; the deep chain runs more sweeps than one launch holds."""
    m, _ = fam(name)
    with Engine(m, lanes_per_node=1) as eng:
        assert eng.info("resident_eligible") == 1 and variants(eng) == {1}
        if flow:
            assert eng.info("flow_eligible") == 1 and eng.info("resident_blocks") > 1
        force(eng, 2, flow)
        check_exact(eng, name, 2, flow)


@pytest.mark.parametrize("name", ["wide5", "wide8", "star"])
def test_one_workgroup_equals_exact(Engine, name):
    m, _ = fam(name)
    with Engine(m) as eng:
        assert eng.info("small_eligible") == 1
        force(eng, 3)
        check_exact(eng, name, 3)


@pytest.mark.parametrize("name", ["arity17", "zeros", "deep", "dagmix", "hub", "group4", "forest14k"])
def test_several_workgroups_equal_exact(Engine, name):
    m, _ = fam(name)
    with Engine(m) as eng:
        assert eng.info("mid_eligible") == 1
        force(eng, 4)
        check_exact(eng, name, 4)
        if name == "forest14k":
            assert eng.info("mid_parts") > 1


DAG = [("wide5", 0), ("zeros", 0), ("deep", 0), ("dagmix", 0), ("hub", 0), ("group4", 0), ("forest", 0), ("forest", 1),
       ("big", 0)]


@pytest.mark.parametrize("name,flow", DAG, ids=[f"{n}-flow{f}" for n, f in DAG])
def test_dag_path_equals_exact(Engine, name, flow):
    """Barrier form, dataflow form (dagflow 1) and stream form ("big": beyond the chip at one tile per wave); arities 2 and
    3 run padded to 4 (dagmix, zeros, deep, hub)."""
    m, _ = fam(name)
    with Engine(m) as eng:
        assert eng.info("dag_eligible") == 1 and eng.info("dag_stream") == (1 if name == "big" else 0)
        force(eng, 5, flow)
        if flow:
            eng.bp_run(Evidence.none(), 0.0, 2)          # (dataflow eligibility is known once the path has been set up)
            assert eng.info("dag_flow_eligible") == 1
        check_exact(eng, name, 5, flow)


# ---- the other entry points --------------------------------------------------------------------

@pytest.mark.parametrize("n_sets", [1, 3, 17])
@pytest.mark.parametrize("name,path", [("zeros", 4), ("zeros", 5), ("forest", 0), ("star", 3)])
def test_batch_equals_exact_per_set(Engine, name, path, n_sets):
    m, _ = fam(name)
    S = X.sweeps_needed(m)
    evs = [X.draw_evidence(m, 3 + q % 7, seed=500 + q, soft=0.4) if q % 5 else Evidence.none() for q in range(n_sets)]
    with Engine(m) as eng:
        force(eng, path)
        out = eng.bp_run_batch(evs, 0.0, S)
        assert eng.last_path() == path
        for q, ev in enumerate(evs):
            assert int(out["sweeps"][q]) == S
            assert np.abs(out["beliefs"][q] - X.exact_marginals(m, ev)[0]).max() <= TOL, q


@pytest.mark.parametrize("name,path", [("zeros", 0), ("zeros", 4), ("wide5", 3), ("dagmix", 5), ("wide9", 0)])
def test_view_equals_exact(Engine, name, path):
    m, _ = fam(name)
    with Engine(m) as eng:
        force(eng, path)
        check_exact(eng, name, path, view=True)


@pytest.mark.parametrize("name,path", [("dagmix", 5), ("dagmix", 4), ("zeros", 0), ("wide12", 0), ("arity17", 4)])
def test_reload_equals_exact_for_the_new_tables(Engine, name, path):
    m, evs = fam(name)
    rng = np.random.default_rng(77)
    cpts = [X._random_table(rng, m.cpt_of(v).shape[0], int(m.k[v]), 0.2) for v in range(m.n)]
    m2 = from_parent_lists(m.k, [m.parents(v) for v in range(m.n)], cpts)
    S = X.sweeps_needed(m)
    ev = X.draw_evidence(m2, 5, seed=3, soft=0.5)
    with Engine(m) as eng:
        force(eng, path)
        eng.bp_run(evs[0], 0.0, S)
        eng.reload_cpt(m2.cpt)
        r = eng.bp_run(ev, 0.0, S)
        assert eng.last_path() == path and r["sweeps"] == S
        assert np.abs(r["beliefs"] - X.exact_marginals(m2, ev)[0]).max() <= TOL


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("name", ["zeros", "arity17", "wide9"])
def test_shards_equal_exact(bnlib, name, nranks):
    from bayesiannetwork_amd import engine
    m, evs = fam(name)
    S = X.sweeps_needed(m)
    for i, ev in enumerate(evs):
        shards = [engine.Engine(m, rank=r, nranks=nranks) for r in range(nranks)]
        try:
            out = engine.run_shards_on_one_device(shards, ev, 0.0, S)
            bel = sum(s.bp_beliefs() for s in shards)
        finally:
            for s in shards:
                s.close()
        assert out["sweeps"] == S
        assert np.abs(bel - exact(name, i)).max() <= TOL


EARLY_PATHS = [(False, 0, 0), (False, 3, 0), (False, 5, 0), (True, 0, 0), (True, 2, 0), (True, 3, 0), (True, 5, 0)]


@pytest.mark.parametrize("uniform,path,flow", EARLY_PATHS, ids=[f"{'k4' if u else 'k23'}-path{p}-flow{f}" for u, p, f in EARLY_PATHS])
def test_early_stop_on_every_path(Engine, uniform, path, flow):
    """The reference's stopping rule (stop after a sweep that changed no message by eps or more; the residual starts at
    DBL_MIN): at eps = 1e-13 every path stops at the oracle's sweep (5) with a bit-identical residual history that ends in
    DBL_MIN, before the beliefs are exact; at S sweeps the history keeps its DBL_MIN entries and the beliefs are exact."""
    m, ev = X.early_stop_case(uniform)
    want = oracle.bp_run(m, ev, 1e-13)
    S = X.sweeps_needed(m)
    pinned = oracle.bp_run(m, ev, 0.0, S)
    assert want["sweeps"] == 5 and want["residuals"][-1] == DBL_MIN
    with Engine(m, lanes_per_node=1 if path == 2 else 0) as eng:
        force(eng, path, flow)
        r = eng.bp_run(ev, 1e-13)
        assert_ran(eng, path, flow)
        assert r["sweeps"] == 5 and np.array_equal(eng.bp_residuals(), want["residuals"])
        assert np.array_equal(r["beliefs"], want["beliefs"])
        r = eng.bp_run(ev, 0.0, S)
        assert_ran(eng, path, flow)
        assert r["sweeps"] == S and np.array_equal(eng.bp_residuals(), pinned["residuals"])
        assert np.abs(r["beliefs"] - X.exact_marginals(m, ev)[0]).max() <= TOL


# ---- likelihood weighting and rejection sampling -----------------------------------------------

def _hard(model, n_ev, seed):
    st = np.full(model.n, -1, dtype=np.int32)
    ev = X.draw_evidence(model, n_ev, seed=seed)
    st[ev.node] = ev.hard_states(model)[ev.node]
    return st


def _lw_band(hist, joint, n):
    est = hist / n
    dev = np.abs(est - joint) - (6.0 * np.sqrt(joint / n) + 1e-12)
    assert dev.max() <= 0, (float(dev.max()), int(np.argmax(dev)))


def _loopy(seed):
    from bayesiannetwork_amd import synth
    return synth.random_dag(16, 3, 8, [2, 3, 2, 4], seed=seed)


LW = [  # name, model factory, exact joint, small kernel expected, BN_LW_SMALL, samples
    ("poly_small", lambda: X.polytree(200, (2, 3, 4), 3, 4, zero_frac=0.2, seed=21), "tree", 1, None, 2_000_000),
    ("poly_generic_env", lambda: X.polytree(200, (2, 3, 4), 3, 4, zero_frac=0.2, seed=21), "tree", 0, "0", 2_000_000),
    ("loopy_small", lambda: _loopy(5), "einsum", 1, None, 4_000_000),
    ("loopy_generic_env", lambda: _loopy(6), "einsum", 0, "0", 1_000_000),
    ("wide16", lambda: fam("wide16")[0], "tree", 0, None, 2_000_000),
    ("arity255", lambda: fam("arity255")[0], "tree", 0, None, 10_000_000),
    ("arity17_k1", lambda: fam("arity17")[0], "tree", 0, None, 4_000_000),   # one-state nodes staged in the generic kernel
]


@pytest.mark.parametrize("name,make,ref,small,env,n", LW, ids=[c[0] for c in LW])
def test_lw_equals_exact_joint(Engine, monkeypatch, name, make, ref, small, env, n):
    if env is not None:
        monkeypatch.setenv("BN_LW_SMALL", env)
    m = make()
    st = _hard(m, 3, seed=9)
    joint = X.exact_joint(m, st) if ref == "tree" else X.einsum_marginals(m, st)[0]
    with Engine(m) as eng:
        hist = eng.lw_run(st, n, seed=20251016)
        assert eng.info("lw_small") == small
    _lw_band(hist, joint, n)


@pytest.mark.parametrize("name,make,ref", [("poly", lambda: X.polytree(60, (2, 3, 4), 3, 4, seed=31), "tree"),
                                            ("loopy", lambda: _loopy(7), "einsum")])
def test_rs_equals_exact_posterior(Engine, name, make, ref):
    m = make()
    st = _hard(m, 2, seed=4)
    if ref == "tree":
        post = X.exact_marginals(m, Evidence.from_dict(m, {v: int(s) for v, s in enumerate(st) if s >= 0}), bp_clamp=False)[0]
    else:
        j, pe = X.einsum_marginals(m, st)
        post = j / pe
    with Engine(m) as eng:
        counts, drawn, acc = eng.rs_run(st, 400_000, seed=77)
    assert acc == 400_000 and drawn >= acc
    est = counts / acc
    assert (np.abs(est - post) <= 6.0 * np.sqrt(post * (1 - post) / acc) + 1e-12).all()
