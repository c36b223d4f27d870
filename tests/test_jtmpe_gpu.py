"""Exact MPE on the junction tree on the GPU (bn_jt_mpe_* of include/bn_mi355x.h; Engine.jt_mpe_run / jt_mpe_run_batch,
JunctionTree.mpe) against the numpy restatement tests/jtmpe_refs.py: states, max-marginals and scale arrays BIT FOR BIT (NaNs as
NaNs), log_p to 1e-12 relative to the sum of the |log scale| (numpy's and the C library's log may differ in the last place).  Both
forms, every evidence kind three times in a row, the tie networks per-node decoding gets wrong, batches whose sets must have the
bits of their single queries, a form-2 batch cut into three launches, the calls around a run, max-product BP beside it, and the
refusals."""
import ctypes

import numpy as np
import pytest

from bayesiannetwork_amd import Evidence, _lib, synth
from bayesiannetwork_amd.engine import Engine, JunctionTree

import jtmpe_refs as jm
import jtree_refs as jr
import maxprod_refs as mr

pytestmark = pytest.mark.gpu

BOTH_FORMS = ["pearl", "alarm", "arity7", "grid3x8"]      # form 1 by the rule; also run with form 2 forced
NATURAL = ["wide12", "grid4x40", "chain3000"]             # form 2 by the rule


def evidence_kinds(m):
    """none; 10 % hard; a soft vector with a zero in it and a strictly positive one; contradictory: an all-zero vector (P(e) = 0)."""
    rng = np.random.default_rng(m.n)
    v = m.n // 2
    w = (v + 1) % m.n
    soft = 0.05 + rng.random(int(m.k[v]))
    soft[0] = 0.0
    return [("none", None), ("hard10", jr.hard_evidence(m, 0.1, 3)),
            ("soft", Evidence.from_dict(m, {v: soft, w: 0.05 + rng.random(int(m.k[w]))})),
            ("contradictory", Evidence.from_dict(m, {v: np.zeros(int(m.k[v]))}))]


@pytest.fixture(scope="module")
def wanted(bnlib):
    """name -> (model, [(kind, evidence, restatement's result)]): computed once, shared, never written."""
    nets, cache = jr.networks(), {}

    def get(name):
        if name not in cache:
            m = nets[name]
            with Engine(m, device=0) as e:
                rs = jm.Restatement(m, e.jt_plan())
            cache[name] = (m, [(kind, ev, rs.run_max(ev)) for kind, ev in evidence_kinds(m)])
        return cache[name]
    return get


def same_log(a, b, scales):
    with np.errstate(divide="ignore"):
        terms = np.abs(np.log(scales))
    return a == b or abs(a - b) <= 1e-12 * float(terms[np.isfinite(terms)].sum())


def check_run(got, want, what):
    states, mm, scales, lg = want
    assert got["states"].dtype == np.int32 and np.array_equal(got["states"], states), (what, "states")
    assert jr.same_bits(got["max_marginals"], mm), (what, "max-marginals", float(np.nanmax(np.abs(got["max_marginals"] - mm))))
    assert jr.same_bits(got["scales"], scales), (what, "scales")
    assert same_log(got["log_p"], lg, scales), (what, got["log_p"], lg)


def run_kinds(wanted, name, form, forced):
    m, cases = wanted(name)
    with Engine(m, device=0) as e:
        if forced:
            e.set_option("jt_form", form)
        assert e.info("jt_form") == form
        for kind, ev, want in cases:
            for rep in range(3):
                check_run(e.jt_mpe_run(ev), want, (name, kind, rep))
            assert e.info("jt_last_form") == form and e.info("jt_last_kind") == 2 and e.info("jt_last_launches") == 1
            if kind == "contradictory":
                v, off = m.n // 2, m.node_off
                assert want[3] == -np.inf and np.isnan(want[1][off[v]:off[v + 1]]).all()
            elif kind != "soft":
                # (chain3000: a table 1 500 levels below the root carries the product of the scales on its path, which underflows --
                # deep nodes' max-marginals are 0 / 0 there, in the restatement and on the device alike; the picks read the tables
                # as collect left them, so the states and log_p stand: DESIGN 4.19)
                assert np.isfinite(want[3]) and (name == "chain3000" or np.isfinite(want[1]).all())
            if kind == "hard10":
                hs = ev.hard_states(m)
                assert np.array_equal(want[0][hs >= 0], hs[hs >= 0])
                jm.check_large(m, ev, want[0], want[1], want[3])   # the decoded assignment is a maximiser


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", BOTH_FORMS)
def test_equals_the_restatement_in_both_forms(wanted, name, form):
    run_kinds(wanted, name, form, forced=form == 2)


@pytest.mark.parametrize("name", NATURAL)
def test_equals_the_restatement_in_form2(wanted, name):
    run_kinds(wanted, name, 2, forced=False)


def test_tie_cases_decode_to_a_maximiser(bnlib):
    m = jm.tie_pair()
    with Engine(m, device=0) as e:
        want = jm.Restatement(m, e.jt_plan()).run_max(None)
        got = e.jt_mpe_run()
        check_run(got, want, "tie pair")
        assert got["states"].tolist() == [0, 1] and got["log_p"] == np.log(0.5) and got["max_marginals"].tolist() == [0.5] * 4
    g = jm.tie_grid()
    for form in (1, 2):
        with Engine(g, device=0) as e:
            e.set_option("jt_form", form)
            want = jm.Restatement(g, e.jt_plan()).run_max(None)
            got = e.jt_mpe_run()
            check_run(got, want, ("tie grid", form))
            assert got["states"].tolist() == [0] * 9


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", sorted(jm.forest_cases()))
def test_forests_equal_the_restatement_in_both_forms(bnlib, name, form):
    """Roots only (one level: the states pay their own barrier), and a childless root beside a deeper tree."""
    m = jm.forest_cases()[name]
    with Engine(m, device=0) as e:
        e.set_option("jt_form", form)
        plan = e.jt_plan()
        assert plan["levels"] == (2 if name == "forest" else 1) and list(plan["parent"]).count(-1) == min(m.n, 2)
        rs = jm.Restatement(m, plan)
        for kind, ev in jm.forest_evidence(m):
            check_run(e.jt_mpe_run(ev), rs.run_max(ev), (name, kind, form))
            assert e.info("jt_last_form") == form and e.info("jt_last_kind") == 2


@pytest.fixture(scope="module")
def alarm_singles(bnlib):
    m = jr.alarm()
    evs = [None] + [jr.hard_evidence(m, f, s) for f, s in ((0.1, 3), (0.3, 4), (0.2, 5))] + [e for _, e in evidence_kinds(m)[2:]]
    with Engine(m, device=0) as e:
        rs = jm.Restatement(m, e.jt_plan())
        singles = [e.jt_mpe_run(ev) for ev in evs]
        for ev, s in zip(evs, singles):
            check_run(s, rs.run_max(ev), "single")
    return m, evs, singles


def same_as_single(got, q, s):
    return (np.array_equal(got["states"][q], s["states"]) and jr.same_bits(got["max_marginals"][q], s["max_marginals"])
            and jr.same_bits(got["scales"][q], s["scales"]) and got["log_p"][q] == s["log_p"])


@pytest.mark.parametrize("n_sets", [1, 2, 257])
def test_batch_sets_have_the_bits_of_their_single_queries(alarm_singles, n_sets):
    m, evs, singles = alarm_singles
    which = [(5 * q + q // 7) % len(evs) for q in range(n_sets)]
    with Engine(m, device=0) as e:
        got = e.jt_mpe_run_batch([evs[i] for i in which])
        assert e.info("jt_last_form") == 1 and e.info("jt_last_launches") == 1 and e.info("jt_last_kind") == 2
    assert got["states"].shape == (n_sets, m.n) and got["states"].dtype == np.int32
    for q, i in enumerate(which):
        assert same_as_single(got, q, singles[i]), q


def test_form2_batch_cut_into_three_launches(wanted):
    m, cases = wanted("grid4x40")
    evs = [None, cases[1][1], jr.hard_evidence(m, 0.3, 4), cases[2][1], jr.hard_evidence(m, 0.2, 5)]
    with Engine(m, device=0) as e:
        singles = [e.jt_mpe_run(ev) for ev in evs]
        e.set_option("jt_scratch_cells", 2 * e.info("jt_state_cells"))   # two sets per launch
        got = e.jt_mpe_run_batch(evs)
        assert e.info("jt_last_form") == 2 and e.info("jt_last_launches") == 3 and e.info("jt_last_kind") == 2
    for q, s in enumerate(singles):
        assert same_as_single(got, q, s), q
    check_run(singles[1], cases[1][2], "grid4x40 hard10")


def test_interleaved_with_the_other_calls(bnlib):
    """jt_run, jt_mpe_run, bp_run, mpe_run, jt_run on one engine: each result has its stand-alone bits; jt_last_kind and the
    scales follow the last junction-tree call."""
    m = jr.alarm()
    ev = jr.hard_evidence(m, 0.2, 9)

    def alone(call):
        with Engine(m, device=0) as e:
            return call(e)
    jt0 = alone(lambda e: e.jt_run(ev))
    mx0 = alone(lambda e: e.jt_mpe_run(ev))
    bp0 = alone(lambda e: e.bp_run(ev, 1e-6))
    lp0 = alone(lambda e: e.mpe_run(ev, 1e-6, 40))
    with Engine(m, device=0) as e:
        assert e.info("jt_last_kind") == 0
        a = e.jt_run(ev)
        assert e.info("jt_last_kind") == 1 and jr.same_bits(e.jt_scales(0), jt0["scales"])
        b = e.jt_mpe_run(ev)
        assert e.info("jt_last_kind") == 2 and jr.same_bits(e.jt_scales(0), mx0["scales"])
        c = e.bp_run(ev, 1e-6)
        d = e.mpe_run(ev, 1e-6, 40)
        assert e.info("jt_last_kind") == 2 and jr.same_bits(e.jt_scales(0), mx0["scales"])
        f = e.jt_run(ev)
        assert e.info("jt_last_kind") == 1 and jr.same_bits(e.jt_scales(0), jt0["scales"])
    for got in (a, f):
        assert jr.same_bits(got["beliefs"], jt0["beliefs"]) and jr.same_bits(got["scales"], jt0["scales"]) and got["log_evidence"] == jt0["log_evidence"]
    assert np.array_equal(b["states"], mx0["states"]) and jr.same_bits(b["max_marginals"], mx0["max_marginals"])
    assert jr.same_bits(b["scales"], mx0["scales"]) and b["log_p"] == mx0["log_p"]
    assert not jr.same_bits(mx0["scales"], jt0["scales"])
    assert jr.same_bits(c["beliefs"], bp0["beliefs"]) and c["sweeps"] == bp0["sweeps"]
    assert np.array_equal(d["states"], lp0["states"]) and jr.same_bits(d["max_marginals"], lp0["max_marginals"]) and d["sweeps"] == lp0["sweeps"]


@pytest.mark.parametrize("case", mr.POLYTREE_CASES, ids=lambda c: "n%d_s%d_e%d" % c)
def test_states_equal_max_product_on_polytrees(bnlib, case):
    m, ev, _ = mr.polytree_case(*case)
    with Engine(m, device=0) as e:
        loopy = e.mpe_run(ev, 1e-9)
        exact = e.jt_mpe_run(ev)
    assert loopy["converged"] and np.array_equal(exact["states"], loopy["states"])


def test_states_differ_from_max_product_on_the_tie_network(bnlib):
    m = jm.tie_pair()
    with Engine(m, device=0) as e:
        loopy = e.mpe_run(None, 1e-9)
        exact = e.jt_mpe_run()
    assert not np.array_equal(exact["states"], loopy["states"])
    logp = lambda st: float(jm._log_terms(m, st, {}).sum())   # noqa: E731
    assert logp(loopy["states"]) == -np.inf and logp(exact["states"]) == exact["log_p"] == np.log(0.5)


def test_junction_tree_class_mpe(bnlib):
    m = synth.pearl()
    jt = JunctionTree(m, device=0)
    try:
        states, logp = jt.mpe({3: 0})
        _, st_want, best, _ = jm.enumerate_mpe(m, Evidence.from_dict(m, {3: 0}))
        assert np.array_equal(states, st_want) and abs(logp - np.log(best)) <= 1e-12 * abs(np.log(best))
        assert states[3] == 0
    finally:
        jt.engine.close()


def test_refusals(bnlib):
    with Engine(synth.grid(8, 8, 4, seed=1), device=0) as e:
        with pytest.raises(_lib.BnError) as err:
            e.jt_mpe_run()
        assert err.value.code == _lib.BN_ERR_STATE and "elimination clique of node" in str(err.value) and "above the limit of 1048576" in str(err.value)
    with Engine(synth.grid(4, 40, 4, seed=1), device=0) as e:
        e.set_option("jt_form", 1)
        with pytest.raises(_lib.BnError) as err:
            e.jt_mpe_run()
        assert err.value.code == _lib.BN_ERR_STATE and "option jt_form = 1" in str(err.value)
        with pytest.raises(_lib.BnError) as err:
            e.jt_mpe_run_batch([None, None])
        assert err.value.code == _lib.BN_ERR_STATE
    m = synth.pearl()
    L = _lib.lib()
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))   # noqa: E731
    mm, st, lg = np.zeros(int(m.k.sum())), np.zeros(m.n, np.int32), ctypes.c_double(0.0)
    node, off, val = np.asarray([3], np.int32), np.asarray([0, 3], np.int32), np.asarray([1.0, 0.0, 0.0])   # three values for a binary node
    with Engine(m, device=_lib.BN_DEVICE_HOST_ONLY) as e:
        rc = L.bn_jt_mpe_run(e._h, 1, p(node, ctypes.c_int32), p(off, ctypes.c_int32), p(val, ctypes.c_double), p(mm, ctypes.c_double),
                             p(st, ctypes.c_int32), ctypes.byref(lg))
        assert rc == _lib.BN_ERR_ARG
        with pytest.raises(_lib.BnError) as err:
            e.jt_mpe_run()
        assert err.value.code == _lib.BN_ERR_NO_DEVICE
