"""The host restatement of exact expectation-maximisation (tests/jtem_refs.py) checked on the CPU, over the plan the library builds
on a BN_DEVICE_HOST_ONLY engine, and what the bn_jt_em_* entry points answer on an engine without a GPU.

- family posteriors against the enumeration of the joint in long double, to 1e-12, and log P(e) from the scales within
  1e-12 x max(1, |log P(e)|): Pearl's network (a polytree) and three networks with loops, the rows of
  em_refs.sampled_table(m, 12, 0.4, seed=77) plus one fully missing row.  The same tables through em_refs.family_posteriors
  (belief propagation at eps = 1e-9) are printed beside them: exact on the polytree, off by 0.006 .. 0.07 on the loopy networks;
- on a complete table E is the integer family counts exactly, and one iteration with prior = 0 has the bits of pattern_refs' CPT fit;
- L, the observed-data log-likelihood the E-step reports from its scales, never falls in 8 iterations on the three cases of
  jtem_refs.likelihood_cases() (smallest increases seen: 0.01486, 1.2088, 0.2649);
- argument and state errors of the entry points on a BN_DEVICE_HOST_ONLY engine."""
import ctypes

import numpy as np
import pytest

import em_refs
import jtem_refs
import pattern_refs
from bayesiannetwork_amd import synth

TOL = 1e-12


@pytest.fixture(scope="module")
def host(bnlib):
    from bayesiannetwork_amd import _lib, engine
    return lambda m, **kw: engine.Engine(m, device=_lib.BN_DEVICE_HOST_ONLY, **kw)


def _plan(host, model):
    with host(model) as e:
        assert e.info("jt_eligible") == 1
        return e.jt_plan()


@pytest.mark.parametrize("name", ["pearl", "grid3x3k2", "grid3x3k4", "dag12"])
def test_family_posteriors_against_enumeration(host, name):
    model = jtem_refs.enumeration_networks()[name]
    pats = jtem_refs.enumeration_table(model)
    assert (pats[-1] == em_refs.MISSING).all() and 2 <= len(pats) <= 13
    step = jtem_refs.ExactE(model, _plan(host, model))
    jnt = jtem_refs.joint(model)
    worst = worst_bp = worst_ll = 0.0
    for row in pats:
        b, skipped, scales = step.row(row)
        want, log_pe = jtem_refs.enumerated_row(model, jnt, row)
        assert skipped == 0
        worst = max(worst, float(np.abs(b - want).max()))
        err = abs(jtem_refs.row_loglik(scales) - float(log_pe))
        worst_ll = max(worst_ll, err / max(1.0, abs(float(log_pe))))
        bp, _ = em_refs.family_posteriors(model, em_refs.bp_run(model, em_refs.evidence_of(model, row), 1e-9, 0))
        worst_bp = max(worst_bp, float(np.abs(bp - want).max()))
    print(f"{name}: max |b - enumeration| = {worst:.3e} (belief propagation: {worst_bp:.3e}), log P(e) relative {worst_ll:.3e}")
    assert worst <= TOL and worst_ll <= TOL


def _family_counts(model, pats, counts):
    out = np.zeros(int(model.cpt_off[-1]), np.uint64)
    for v in range(model.n):
        row = np.zeros(len(counts), np.int64)
        for u in model.parents(v):
            row = row * int(model.k[u]) + pats[:, int(u)]
        np.add.at(out, int(model.cpt_off[v]) + row * int(model.k[v]) + pats[:, v], counts)
    return out


@pytest.mark.parametrize("name", ["grid3x3k2", "dag12"])
def test_complete_table_gives_the_counts_and_the_cpt_fit(host, name):
    model = jtem_refs.enumeration_networks()[name]
    pats, counts = em_refs.sampled_table(model, 300, 0.0, seed=51)
    counts = counts * np.uint64(3) + np.uint64(1)
    assert (pats != em_refs.MISSING).all() and (model.cpt > 0).all()
    plan = _plan(host, model)
    e = jtem_refs.expected_counts(model, plan, pats, counts)
    assert e["skipped"] == 0
    assert np.array_equal(e["E"], _family_counts(model, pats, counts).astype(np.float64))
    fit = jtem_refs.em_fit(model, plan, pats, counts, max_iters=1, tol=0.0, prior=0.0)
    assert fit["iters"] == 1
    assert np.array_equal(fit["cpt"], pattern_refs.fit_cpt_ref(model, pats, counts))


@pytest.mark.parametrize("case", range(3))
def test_loglik_never_falls(host, case):
    model, n_samples, blank, table_seed, init_seed = jtem_refs.likelihood_cases()[case]
    pats, counts = em_refs.sampled_table(model, n_samples, blank, seed=table_seed)
    init = em_refs.random_positive_cpt(model, init_seed)
    fit = jtem_refs.em_fit(model, _plan(host, model), pats, counts, max_iters=8, tol=0.0, cpt_init=init)
    assert fit["iters"] == 8 and fit["skipped"] == 0
    # L of iteration i is the likelihood of the tables it started from: the ninth value is that of the tables the loop ends with
    last = jtem_refs.expected_counts(em_refs.with_cpt(model, fit["cpt"]), _plan(host, model), pats, counts)["L"]
    ll = np.asarray(fit["L"] + [last])
    inc = np.diff(ll)
    print(f"case {case} ({model.name}): L {ll[0]:.4f} -> {ll[-1]:.4f}, smallest increase {inc.min():.6g}")
    assert (inc > 0).all(), inc


# ---- the entry points without a GPU ---------------------------------------------------------------------------------------------

def _fit_raw(e, pats, counts, max_iters=5, tol=1e-6, prior=0.0, opt=True, out=True, n_patterns=None):
    from bayesiannetwork_amd import _lib
    L = _lib.lib()
    u8, u64, f64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
    pats = None if pats is None else np.ascontiguousarray(pats, np.uint8)
    counts = None if counts is None else np.ascontiguousarray(counts, np.uint64)
    o = _lib.JtEmOptions(max_iters, tol, prior)
    cpt = np.zeros(int(e.model.cpt_off[-1]))
    P = n_patterns if n_patterns is not None else (0 if pats is None else pats.reshape(-1, e.model.n).shape[0])
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    rc = L.bn_jt_em_fit(e._h, P, p(pats, u8), p(counts, u64), ctypes.byref(o) if opt else None, None, p(cpt, f64) if out else None, None, None,
                        None, 0)
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
    assert _fit_raw(e, ok_p, ok_c, tol=float("nan"))[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, None, ok_c, n_patterns=2)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, None)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, ok_c, opt=False)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, ok_c, out=False)[0] == _lib.BN_ERR_ARG
    assert _fit_raw(e, ok_p, ok_c, n_patterns=0)[0] == _lib.BN_ERR_ARG
    # well-formed arguments pass the checks and reach the "no GPU" answer
    rc, msg = _fit_raw(e, ok_p, ok_c)
    assert rc == _lib.BN_ERR_NO_DEVICE and "BN_DEVICE_HOST_ONLY" in msg
    with pytest.raises(_lib.BnError) as err:
        e.jt_em_expected_counts(ok_p, ok_c)
    assert err.value.code == _lib.BN_ERR_NO_DEVICE
    with pytest.raises(_lib.BnError) as err:
        e.jt_em_expected_counts([[0, 3, 0, 0]], [1])
    assert err.value.code == _lib.BN_ERR_ARG and "pattern 0" in str(err.value) and "node 1" in str(err.value)
    assert e.info("jt_last_kind") == 0 and e.info("jt_em_last_iters") == 0


def test_ineligible_network_is_a_state_error_with_the_planners_reason(host):
    from bayesiannetwork_amd import _lib
    m = synth.grid(8, 8, 4, seed=1)
    e = host(m)
    pats, counts = np.full((1, m.n), 255, np.uint8), np.asarray([1], np.uint64)
    rc, msg = _fit_raw(e, pats, counts)
    assert rc == _lib.BN_ERR_STATE and "elimination clique" in msg, msg
    bad = pats.copy()
    bad[0, 5] = 4
    rc, msg = _fit_raw(e, bad, counts)   # the argument check comes first
    assert rc == _lib.BN_ERR_ARG and "pattern 0" in msg and "node 5" in msg, msg
    with pytest.raises(_lib.BnError) as err:
        e.jt_em_expected_counts(pats, counts)
    assert err.value.code == _lib.BN_ERR_STATE and "elimination clique" in str(err.value)


def test_option_and_info_names(host):
    from bayesiannetwork_amd import _lib
    e = host(synth.pearl())
    assert e.info("jt_em_scratch_cells") == 1 << 22
    e.set_option("jt_em_scratch_cells", 1000)
    assert e.info("jt_em_scratch_cells") == 1000
    e.set_option("jt_em_scratch_cells", 0)
    assert e.info("jt_em_scratch_cells") == 1 << 22
    with pytest.raises(_lib.BnError):
        e.set_option("jt_em_scratch_cells", -1)
    for name in ("jt_em_last_iters", "jt_em_skipped", "jt_em_estep_ns", "jt_em_mstep_ns", "jt_em_last_form", "jt_em_last_launches"):
        assert e.info(name) == 0
