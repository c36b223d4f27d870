"""The host restatement of expectation-maximisation (tests/em_refs.py) checked on the CPU, and what the bn_em_* entry points answer on
an engine without a GPU.

- its belief-propagation loop is maxprod_refs.run(mode="sum") bit for bit: beliefs, messages, sweep counts, residuals;
- the family posteriors b[a,i] are P(x_v = i, pa(v) = a | e) by enumeration of the joint on the polytrees of
  maxprod_refs.POLYTREE_CASES, within the 1e-12 tests/test_exact_gpu.py holds belief propagation to on polytrees;
- on a complete table E is the integer family counts exactly, and one iteration with prior = 0 has the bits of pattern_refs' CPT fit;
- EM raises the observed-data log-likelihood (exact_refs.exact_marginals, long double) at every one of 8 iterations on the cases of
  em_refs.LIKELIHOOD_CASES.  Smallest per-iteration increase observed over those cases: 0.0734 (case (8, 2, 200, 0.3, 12));
- argument and state errors of bn_em_expected_counts / bn_em_fit on a BN_DEVICE_HOST_ONLY engine.
"""
import ctypes

import numpy as np
import pytest

import em_refs
import exact_refs
import maxprod_refs
import pattern_refs
from bayesiannetwork_amd import Evidence, from_parent_lists, synth
from bayesiannetwork_amd.dsc import load_dsc

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _same_run(model, ev, eps, cap):
    want = maxprod_refs.run(model, ev, eps, cap, mode="sum")
    got = em_refs.bp_run(model, ev, eps, cap)
    assert got["sweeps"] == want["sweeps"] and got["converged"] == want["converged"]
    assert np.array_equal(got["residuals"], want["residuals"])
    for key in ("beliefs", "pi_msg", "lambda_msg"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key


@pytest.mark.parametrize("n,seed,n_ev", maxprod_refs.POLYTREE_CASES)
def test_bp_loop_is_the_pinned_one_on_polytrees(n, seed, n_ev):
    model, ev, _ = maxprod_refs.polytree_case(n, seed, n_ev)
    _same_run(model, ev, 1e-13, 60)
    _same_run(model, ev, 1e-3, 2)


def test_bp_loop_is_the_pinned_one_on_loopy_networks():
    alarm = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    _same_run(alarm, synth.random_evidence(alarm, 0.2, seed=3), 1e-6, 40)
    grid = synth.grid(3, 3, 3, seed=4)
    _same_run(grid, Evidence.from_dict(grid, {4: 1}), 1e-9, 3)


def _family_by_enumeration(model, ev_state, v):
    """P(x_v, pa(v) | e) as a [rows, k_v] table: the joint over the free nodes summed down to the family, evidence members at their state."""
    joint, free = maxprod_refs.joint_tensor(model, ev_state)
    fam = [int(u) for u in model.parents(v)] + [v]
    keep = [a for a, u in enumerate(free) if u in fam]
    marg = joint.sum(axis=tuple(a for a in range(len(free)) if a not in keep)) if free else joint
    marg = np.asarray(marg, dtype=np.float64) / float(joint.sum())
    kept_nodes = [free[a] for a in keep]                     # ascending ids: the axes of `marg`
    out = np.zeros([int(model.k[u]) for u in fam])
    idx = tuple(int(ev_state[u]) if ev_state[u] >= 0 else slice(None) for u in fam)
    free_in_fam = [u for u in fam if ev_state[u] < 0]        # order of the axes `out[idx]` keeps
    out[idx] = np.transpose(marg, [kept_nodes.index(u) for u in free_in_fam]) if free_in_fam else marg
    return out.reshape(-1, int(model.k[v]))


@pytest.mark.parametrize("n,seed,n_ev", maxprod_refs.POLYTREE_CASES)
def test_family_posteriors_are_posteriors(n, seed, n_ev):
    model, ev, ev_state = maxprod_refs.polytree_case(n, seed, n_ev)
    run = em_refs.bp_run(model, ev, 1e-13, 0)
    assert run["converged"]
    b, skipped = em_refs.family_posteriors(model, run)
    assert skipped == 0
    worst = 0.0
    for v in range(model.n):
        want = _family_by_enumeration(model, ev_state, v)
        got = b[int(model.cpt_off[v]):int(model.cpt_off[v + 1])].reshape(want.shape)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"polytree n={n} seed={seed} evidence={n_ev}: max |b - enumeration| = {worst:.3e}")
    assert worst <= TOL


def _family_counts(model, pats, counts):
    out = np.zeros(int(model.cpt_off[-1]), np.uint64)
    for v in range(model.n):
        row = np.zeros(len(counts), np.int64)
        for u in model.parents(v):
            row = row * int(model.k[u]) + pats[:, int(u)]
        np.add.at(out, int(model.cpt_off[v]) + row * int(model.k[v]) + pats[:, v], counts)
    return out


@pytest.mark.parametrize("n,seed", [(8, 1), (10, 3)])
def test_complete_table_gives_the_counts_and_the_cpt_fit(n, seed):
    model = exact_refs.polytree(n, arities=(2, 3, 4), max_parents=3, seed=seed)
    pats, counts = em_refs.sampled_table(model, 300, 0.0, seed=50 + seed)
    counts = counts * np.uint64(3) + np.uint64(1)
    assert (pats != em_refs.MISSING).all() and (model.cpt > 0).all()
    e = em_refs.expected_counts(model, pats, counts, 1e-3, 0)
    assert e["skipped"] == 0 and e["capped"] == 0
    assert np.array_equal(e["E"], _family_counts(model, pats, counts).astype(np.float64))
    fit = em_refs.em_fit(model, pats, counts, max_iters=1, tol=0.0, prior=0.0)
    assert fit["iters"] == 1
    assert np.array_equal(fit["cpt"], pattern_refs.fit_cpt_ref(model, pats, counts))


@pytest.mark.parametrize("case", em_refs.LIKELIHOOD_CASES)
def test_em_improves_the_likelihood(case):
    model, pats, counts, init = em_refs.likelihood_case(*case)
    assert (init > 0).all() and not np.array_equal(init, model.cpt)
    blanked = float((pats == em_refs.MISSING).mean())
    assert 0.15 <= blanked <= 0.45, blanked
    fit = em_refs.em_fit(model, pats, counts, max_iters=8, tol=0.0, bp_eps=1e-13, bp_max_sweeps=0, cpt_init=init)
    assert fit["iters"] == 8 and fit["capped"] == 0 and fit["skipped"] == 0
    ll = [em_refs.log_likelihood(em_refs.with_cpt(model, th), pats, counts) for th in [init] + fit["thetas"]]
    inc = np.diff(np.asarray(ll, dtype=np.longdouble))
    print(f"case {case}: log-likelihood {float(ll[0]):.4f} -> {float(ll[-1]):.4f}, smallest increase {float(inc.min()):.6g}")
    assert (inc > 0).all(), inc


# ---- the entry points without a GPU ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host(bnlib):
    from bayesiannetwork_amd import _lib, engine
    return lambda m, **kw: engine.Engine(m, device=_lib.BN_DEVICE_HOST_ONLY, **kw)


def _fit_raw(e, pats, counts, max_iters=5, tol=1e-6, prior=0.0, bp_eps=1e-3, bp_max_sweeps=0, opt=True, out=True, n_patterns=None):
    from bayesiannetwork_amd import _lib
    L = _lib.lib()
    u8, u64, f64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    pats = None if pats is None else np.ascontiguousarray(pats, np.uint8)
    counts = None if counts is None else np.ascontiguousarray(counts, np.uint64)
    o = _lib.EmOptions(max_iters, tol, bp_eps, bp_max_sweeps, prior)
    cpt = np.zeros(int(e.model.cpt_off[-1]))
    P = n_patterns if n_patterns is not None else (0 if pats is None else pats.reshape(-1, e.model.n).shape[0])
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    rc = L.bn_em_fit(e._h, P, p(pats, u8), p(counts, u64), ctypes.byref(o) if opt else None, None, p(cpt, f64) if out else None, None, None, 0)
    return rc, L.bn_last_error().decode()


def test_argument_errors_come_before_the_device(host):
    from bayesiannetwork_amd import _lib
    e = host(synth.pearl())   # four binary nodes
    ok_p, ok_c = np.asarray([[0, 1, 255, 1], [255, 255, 255, 255]], np.uint8), np.asarray([3, 2], np.uint64)
    rc, msg = _fit_raw(e, [[0, 1, 2, 1]], [1])
    assert rc == _lib.BN_ERR_ARG and "pattern 0" in msg and "node 2" in msg, msg
    rc, msg = _fit_raw(e, [[0, 1, 1, 1], [0, 254, 0, 0]], [1, 1])
    assert rc == _lib.BN_ERR_ARG and "pattern 1" in msg and "node 1" in msg, msg
    rc, msg = _fit_raw(e, ok_p, [0, 0])
    assert rc == _lib.BN_ERR_ARG and "zero" in msg, msg
    for bad in (0, -1, 10001):
        rc, msg = _fit_raw(e, ok_p, ok_c, max_iters=bad)
        assert rc == _lib.BN_ERR_ARG and "max_iters" in msg, (bad, msg)
    for bad in (-1e-300, -1.0, float("nan"), float("inf")):
        rc, msg = _fit_raw(e, ok_p, ok_c, prior=bad)
        assert rc == _lib.BN_ERR_ARG and "prior" in msg, (bad, msg)
    assert _fit_raw(e, ok_p, ok_c, bp_max_sweeps=-1)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, ok_c, tol=float("nan"))[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, None, ok_c, n_patterns=2)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, None)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, ok_c, opt=False)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, ok_c, out=False)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, ok_c, n_patterns=0)[0] == _lib.BN_ERR_ARG
    # well-formed arguments pass the checks and reach the "no GPU" answer
    rc, msg = _fit_raw(e, ok_p, ok_c)
    assert rc == _lib.BN_ERR_NO_DEVICE and "BN_DEVICE_HOST_ONLY" in msg
    with pytest.raises(_lib.BnError) as ei:
        e.em_fit(ok_p, ok_c, max_iters=3)
    assert ei.value.code == _lib.BN_ERR_NO_DEVICE
    # one E-step: the same checks
    with pytest.raises(_lib.BnError) as ei:
        e.em_expected_counts([[0, 1, 2, 1]], [1])
    assert ei.value.code == _lib.BN_ERR_ARG
    with pytest.raises(_lib.BnError) as ei:
        e.em_expected_counts(ok_p, [0, 0])
    assert ei.value.code == _lib.BN_ERR_ARG
    with pytest.raises(_lib.BnError) as ei:
        e.em_expected_counts(ok_p, ok_c, bp_max_sweeps=-2)
    assert ei.value.code == _lib.BN_ERR_ARG
    with pytest.raises(_lib.BnError) as ei:
        e.em_expected_counts(ok_p, ok_c)
    assert ei.value.code == _lib.BN_ERR_NO_DEVICE
    assert e.info("em_eligible") == 1 and e.info("em_last_iters") == 0 and e.info("em_capped") == 0 and e.info("em_skipped") == 0


def test_networks_without_a_one_workgroup_plan_say_why(host):
    from bayesiannetwork_amd import MISSING, _lib
    assert MISSING == 255
    m = 9
    rng = np.random.default_rng(5)
    t = 0.1 + rng.random((2 ** m, 2))
    model = from_parent_lists(k=[2] * (m + 1), parents=[[] for _ in range(m)] + [list(range(m))],
                              cpts=[[0.5, 0.5]] * m + [(t / t.sum(axis=1, keepdims=True)).ravel().tolist()], name="nine_parents")
    e = host(model)
    assert e.info("em_eligible") == 0
    with pytest.raises(_lib.BnError, match="more than 8 parents") as ei:
        e.em_fit(np.zeros((1, m + 1), np.uint8), [1], max_iters=2)
    assert ei.value.code == _lib.BN_ERR_STATE
    sharded = host(synth.grid(12, 12, 4, seed=2), rank=0, nranks=2)
    assert sharded.info("em_eligible") == 0
    with pytest.raises(_lib.BnError, match="sharded") as ei:
        sharded.em_expected_counts(np.zeros((1, 144), np.uint8), [1])
    assert ei.value.code == _lib.BN_ERR_STATE
    with pytest.raises(_lib.BnError) as ei:
        e.set_option("em_scratch_cells", -1)
    assert ei.value.code == _lib.BN_ERR_ARG
    with pytest.raises(_lib.BnError):
        e.set_option("em_nonsense", 1)
