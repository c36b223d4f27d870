"""bn_gibbs_run on the GPU against the host restatement (tests/gibbs_refs.py): counts, final states, stuck and kept are equal exactly
-- integers and bytes, nothing to tolerate -- on networks that reach every part of the kernel: tables with zeros and stuck updates,
a colour class of 70 slots (more than a wave has lanes: a chain is a whole wave there, 8 or 16 lanes on the small networks), nodes
with 5 and 8 parents and arity 7, arities 9 and 11, chain counts that are no multiple of the chains of a workgroup, chain ids beyond 2^32, no evidence, every node observed, no sweeps, burn-in beyond the run,
thinning, a run split into launches, runs continued across calls, the start against the sampler's own states, reloaded tables; and
the refusals.  Every case is a few chains and sweeps: a fraction of a second."""
import ctypes

import numpy as np
import pytest

from bayesiannetwork_amd import _lib, engine, synth

import exact_refs as xr
import gibbs_refs as gr
import jtree_refs as jr
import many_parents
from test_gibbs_refs import PEARL_STUCK_EVIDENCE, ev_of

pytestmark = pytest.mark.gpu

BIG = (1 << 32) + 3     # chain ids whose high word is not zero


def _dag12():
    return synth.random_dag(12, max_parents=3, window=6, k=3, seed=5)


def _grid():
    return synth.grid(3, 3, k=3)


def _alarm_ev(m):
    return {int(v): int(s) for v, s in enumerate(jr.ev_state_of(m, jr.hard_evidence(m, 0.1, 3))) if s >= 0}


# id -> (model, evidence {node: state} or a function of the model, arguments of the run)
CASES = {
    "pearl_stuck": (synth.pearl, PEARL_STUCK_EVIDENCE, dict(n_chains=67, n_sweeps=6, seed=5)),
    "grid3x3": (_grid, {1: 2, 8: 0}, dict(n_chains=64, n_sweeps=8, seed=11)),
    "dag12": (_dag12, {2: 1, 9: 0}, dict(n_chains=64, n_sweeps=8, seed=12)),
    "alarm": (jr.alarm, _alarm_ev, dict(n_chains=64, n_sweeps=8, seed=13)),
    "star70": (lambda: xr.star(70, 3, 2), {5: 1, 70: 0}, dict(n_chains=9, n_sweeps=4, seed=14)),
    "fan5_8": (lambda: many_parents.fan([5, 8], kp=2, kc=7), {10: 1}, dict(n_chains=10, n_sweeps=4, seed=15)),
    # arities above eight: the kernel computes such a node's weights twice instead of keeping them in registers
    "arity11": (lambda: synth.random_dag(14, max_parents=3, window=6, k=[11, 2, 9, 3], seed=4), {1: 1, 12: 5}, dict(n_chains=9, n_sweeps=4, seed=25)),
    "chains1": (_dag12, {2: 1, 9: 0}, dict(n_chains=1, n_sweeps=5, seed=16, chain_begin=BIG)),
    "chains5": (_dag12, {2: 1, 9: 0}, dict(n_chains=5, n_sweeps=5, seed=16, chain_begin=BIG)),
    "chains67": (_dag12, {2: 1, 9: 0}, dict(n_chains=67, n_sweeps=5, seed=(0x9E3779B1 << 32) | 0x7F4A7C15, chain_begin=BIG)),
    "no_evidence": (_grid, {}, dict(n_chains=33, n_sweeps=6, seed=17)),
    "all_observed": (_grid, lambda m: {v: v % 3 for v in range(m.n)}, dict(n_chains=6, n_sweeps=3, seed=18)),
    "no_sweeps": (_dag12, {2: 1, 9: 0}, dict(n_chains=7, n_sweeps=0, seed=19)),
    "burn_in_beyond": (_dag12, {2: 1, 9: 0}, dict(n_chains=7, n_sweeps=4, seed=20, burn_in=9)),
    "thin3": (_dag12, {2: 1, 9: 0}, dict(n_chains=7, n_sweeps=11, seed=21, burn_in=2, thin=3, sweep_begin=1)),
}


def _same(got, want):
    assert got["kept"] == want["kept"] and got["stuck"] == want["stuck"], (got["kept"], want["kept"], got["stuck"], want["stuck"])
    assert got["states"].dtype == np.uint8 and np.array_equal(got["states"], want["states"])
    assert got["counts"].dtype == np.uint64 and np.array_equal(got["counts"], want["counts"])


def _case(name):
    make, ev, kw = CASES[name]
    m = make()
    return m, ev_of(m, ev(m) if callable(ev) else ev), kw


@pytest.mark.parametrize("name", list(CASES))
def test_run_equals_the_restatement(name, bnlib, oracle_mod):
    m, ev, kw = _case(name)
    want = gr.run(m, ev, oracle=oracle_mod, **kw)
    with engine.Engine(m, device=0) as e:
        got = e.gibbs_run(ev, **kw)
        assert e.info("gibbs_last_launches") == (1 if kw["n_sweeps"] else 0)
    _same(got, want)
    if name == "pearl_stuck":
        assert got["stuck"] > 0
    if name in ("no_sweeps", "burn_in_beyond"):
        assert got["kept"] == 0 and not got["counts"].any()
    if name == "all_observed":
        assert (got["states"] == ev.astype(np.uint8)).all() and got["kept"] == 18


def test_split_into_launches_changes_no_bit(bnlib, oracle_mod):
    m, ev = _dag12(), ev_of(_dag12(), {2: 1, 9: 0})
    kw = dict(n_chains=13, n_sweeps=10, seed=22, burn_in=1, thin=2)
    want = gr.run(m, ev, oracle=oracle_mod, **kw)
    with engine.Engine(m, device=0) as e:
        one = e.gibbs_run(ev, **kw)
        assert e.info("gibbs_last_launches") == 1
        e.set_option("gibbs_sweeps_per_launch", 3)
        assert e.info("gibbs_sweeps_per_launch") == 3 and e.gibbs_plan()["sweeps_per_launch"] == 3
        split = e.gibbs_run(ev, **kw)
        assert e.info("gibbs_last_launches") == 4
    _same(one, want)
    _same(split, want)


def test_runs_continue_across_calls_and_chain_ranges_add_up(bnlib, oracle_mod):
    m, ev = _dag12(), ev_of(_dag12(), {2: 1, 9: 0})
    kw = dict(seed=77, burn_in=2, thin=3, chain_begin=BIG)
    with engine.Engine(m, device=0) as e:
        whole = e.gibbs_run(ev, 9, 11, **kw)
        a = e.gibbs_run(ev, 9, 4, **kw)
        b = e.gibbs_run(ev, 9, 7, sweep_begin=4, init_states=a["states"], **kw)
        lo = e.gibbs_run(ev, 5, 11, **kw)
        hi = e.gibbs_run(ev, 4, 11, **dict(kw, chain_begin=BIG + 5))
    _same(whole, gr.run(m, ev, 9, 11, oracle=oracle_mod, **kw))
    assert np.array_equal(b["states"], whole["states"])
    assert np.array_equal(a["counts"] + b["counts"], whole["counts"])
    assert a["kept"] + b["kept"] == whole["kept"] and a["stuck"] + b["stuck"] == whole["stuck"]
    assert np.array_equal(np.concatenate([lo["states"], hi["states"]]), whole["states"])
    assert np.array_equal(lo["counts"] + hi["counts"], whole["counts"])


def test_init_states_are_used_and_evidence_nodes_overwritten(bnlib, oracle_mod):
    m, ev = _dag12(), ev_of(_dag12(), {2: 1, 9: 0})
    init = np.random.default_rng(3).integers(0, 3, size=(6, m.n)).astype(np.uint8)
    init[:, 2] = 2      # contradicts the evidence: overwritten by the clamp
    kw = dict(n_chains=6, n_sweeps=3, seed=23, init_states=init)
    with engine.Engine(m, device=0) as e:
        got = e.gibbs_run(ev, **kw)
        start = e.gibbs_run(ev, **dict(kw, n_sweeps=0))
    _same(got, gr.run(m, ev, **kw))
    want_start = init.copy()
    want_start[:, 2], want_start[:, 9] = 1, 0
    assert np.array_equal(start["states"], want_start)


def test_start_equals_the_samplers_states(bnlib):
    m = jr.alarm()
    ev = ev_of(m, _alarm_ev(m))
    with engine.Engine(m, device=0) as e:
        start = e.gibbs_run(ev, 70, 0, seed=31, chain_begin=BIG)["states"]
        e.lw_run(ev, 70, 31, sample_begin=BIG)
        states, _ = e.lw_states(70)
    assert np.array_equal(start, states)


def test_reloaded_tables_are_read(bnlib, oracle_mod):
    m, ev = _dag12(), ev_of(_dag12(), {2: 1, 9: 0})
    kw = dict(n_chains=9, n_sweeps=5, seed=24)
    rng = np.random.default_rng(9)
    cpt = np.asarray(m.cpt, dtype=np.float64).copy()
    for v in range(m.n):        # other tables on the same structure: every row redrawn and normalised
        rows = cpt[m.cpt_off[v]:m.cpt_off[v + 1]].reshape(-1, int(m.k[v]))
        rows[:] = 0.1 + rng.random(rows.shape)
        rows /= rows.sum(axis=1, keepdims=True)
    m2 = type(m)(k=m.k.copy(), in_ptr=m.in_ptr.copy(), in_idx=m.in_idx.copy(), cpt_off=m.cpt_off.copy(), cpt=cpt)
    with engine.Engine(m, device=0) as e:
        before = e.gibbs_run(ev, **kw)
        e.reload_cpt(cpt)
        after = e.gibbs_run(ev, **kw)
    _same(before, gr.run(m, ev, oracle=oracle_mod, **kw))
    _same(after, gr.run(m2, ev, oracle=oracle_mod, **kw))
    assert not np.array_equal(before["counts"], after["counts"])


def test_refusals(bnlib):
    from bayesiannetwork_amd import from_parent_lists
    m = _dag12()
    ev = ev_of(m, {2: 1})
    with engine.Engine(m, device=0) as e:
        with pytest.raises(_lib.BnError) as ei:
            e.gibbs_run(ev, 4, 2, seed=1, thin=0)
        assert ei.value.code == _lib.BN_ERR_ARG
        bad = np.zeros((4, m.n), dtype=np.uint8)
        bad[3, 5] = 3       # arity 3: states 0..2
        with pytest.raises(_lib.BnError) as ei:
            e.gibbs_run(ev, 4, 2, seed=1, init_states=bad)
        assert ei.value.code == _lib.BN_ERR_ARG and "node 5" in str(ei.value)
        bad[3, 5], bad[0, 2] = 0, 200       # ... but an evidence node's start state is overwritten, whatever it is
        e.gibbs_run(ev, 4, 2, seed=1, init_states=bad)
        for node, state in ((12, 0), (2, 3)):       # an unknown evidence node, an unknown state (straight at the C call)
            nodes, states = np.array([node], dtype=np.int32), np.array([state], dtype=np.int32)
            out = np.zeros(int(m.k.sum()), dtype=np.uint64)
            with pytest.raises(_lib.BnError) as ei:
                _lib.check(bnlib.bn_gibbs_run(e._h, 1, nodes.ctypes.data_as(_lib.i32p), states.ctypes.data_as(_lib.i32p), 0, 4, 0, 2, 0, 1, 1, None,
                                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, None, None))
            assert ei.value.code == _lib.BN_ERR_ARG
        with pytest.raises(_lib.BnError) as ei:
            e.gibbs_run(ev, 4, 2, seed=1, sweep_begin=(1 << 32) - 1)
        assert ei.value.code == _lib.BN_ERR_ARG
    # 4 097 parentless nodes of one state: refused with the planner's reason, nothing is launched
    n = 4097
    wide = from_parent_lists([1] * n, [[] for _ in range(n)], [[1.0] for _ in range(n)])
    with engine.Engine(wide, device=0) as e:
        assert e.info("gibbs_eligible") == 0
        with pytest.raises(_lib.BnError) as ei:
            e.gibbs_run(np.full(n, -1, np.int32), 4, 2, seed=1)
        assert ei.value.code == _lib.BN_ERR_STATE and "4097 nodes" in str(ei.value)
        assert e.info("gibbs_last_launches") == 0
        with pytest.raises(_lib.BnError) as ei:
            e.gibbs_plan()
        assert ei.value.code == _lib.BN_ERR_STATE and "4097 nodes" in str(ei.value)
