"""Exact MPE on the junction tree (bn_jt_mpe_run) on the CPU: the numpy restatement of its arithmetic (tests/jtmpe_refs.py) over the
plan the library builds on a BN_DEVICE_HOST_ONLY engine, against the enumeration of the joint -- states equal to the argmax, the
max-marginals to 1e-12 absolute, log_p to 1e-12 relative -- on Pearl's network, two grids, a random DAG and the polytree cases of
max-product BP, each without evidence, with two hard nodes and with one soft vector; the tie networks per-node decoding gets wrong;
the networks too large to enumerate by the properties of a maximiser; P(e) = 0; the argument and state errors of the new calls on
an engine without a device."""
import ctypes

import numpy as np
import pytest

from bayesiannetwork_amd import Evidence, _lib, engine, synth

import jtmpe_refs as jm
import jtree_refs as jr
import maxprod_refs as mr


@pytest.fixture(scope="module")
def host_engine(bnlib):
    assert _lib.lib().bn_jt_mpe_run and _lib.lib().bn_jt_mpe_run_batch   # the calls these tests restate
    return lambda m: engine.Engine(m, device=_lib.BN_DEVICE_HOST_ONLY)


def _restate(host_engine, m):
    with host_engine(m) as e:
        return jm.Restatement(m, e.jt_plan())


def _check_against_enumeration(rs, m, ev, what, want=None):
    mm_want, st_want, best, second = want if want is not None else jm.enumerate_mpe(m, ev)
    assert best > 0 and second < best * (1 - 1e-9), (what, "the case fails the margin", best, second)
    states, mm, scales, lg = rs.run_max(ev)
    dev = float(np.abs(mm - mm_want).max())
    print(what, "max-marginal deviation", dev, "log_p", lg, np.log(best))
    assert np.array_equal(states, st_want), (what, states, st_want)
    assert dev <= 1e-12
    assert abs(lg - np.log(best)) <= 1e-12 * max(1.0, abs(np.log(best)))
    assert abs(np.prod(scales) - best) <= 1e-12 * best


@pytest.mark.parametrize("name", sorted(jm.small_cases()))
def test_restatement_equals_enumeration(host_engine, name):
    m = jm.small_cases()[name]
    rs = _restate(host_engine, m)
    for kind, ev in jm.small_evidence(m):
        _check_against_enumeration(rs, m, ev, (name, kind))
        if kind == "hard2" and name.startswith("polytree"):   # maxprod_refs' own enumeration (it pins itself to a polytree reference)
            mm, st, best, second = mr.brute_max_marginals(m, ev.hard_states(m))
            _check_against_enumeration(rs, m, ev, (name, kind, "brute_max_marginals"), (mm, st, best, second))


@pytest.mark.parametrize("kind", [0, 1], ids=["none", "soft"])
@pytest.mark.parametrize("name", sorted(jm.forest_cases()))
def test_forests_equal_enumeration(host_engine, name, kind):
    """Roots only (one level), and a childless root beside a deeper tree: the decode's two special paths."""
    m = jm.forest_cases()[name]
    with host_engine(m) as e:
        plan = e.jt_plan()
    shape = {"lone": ([-1], [0]), "two": ([-1, -1], [0, 0]), "forest": ([-1, -1, 1], [0, 0, 1])}[name]
    assert (list(plan["parent"]), list(plan["level"])) == shape
    what, ev = jm.forest_evidence(m)[kind]
    _check_against_enumeration(jm.Restatement(m, plan), m, ev, (name, what))


@pytest.mark.parametrize("case", mr.POLYTREE_CASES, ids=lambda c: "n%d_s%d_e%d" % c)
def test_polytree_cases_with_their_own_evidence(host_engine, case):
    m, ev, ev_state = mr.polytree_case(*case)
    _check_against_enumeration(_restate(host_engine, m), m, ev, case, mr.brute_max_marginals(m, ev_state))


def test_tie_pair_decodes_to_a_maximiser(host_engine):
    """Both max-marginals are [0.5, 0.5]: per-node decoding gives (0, 0), probability 0; backtracking gives (0, 1)."""
    m = jm.tie_pair()
    states, mm, _, lg = _restate(host_engine, m).run_max(None)
    assert states.tolist() == [0, 1] and mm.tolist() == [0.5, 0.5, 0.5, 0.5]
    assert lg == np.log(0.5)
    assert [mr.decode(mm[0:2]), mr.decode(mm[2:4])] == [0, 0]


def test_tie_grid_decodes_to_all_zeros(host_engine):
    m = jm.tie_grid()
    states, mm, _, lg = _restate(host_engine, m).run_max(None)
    assert states.tolist() == [0] * 9 and np.array_equal(mm, np.full(18, 0.5))
    assert abs(lg - 9 * np.log(0.5)) <= 1e-12 * 9 * abs(np.log(0.5))


@pytest.mark.parametrize("name", ["alarm", "grid4x40", "star", "wide12", "chain3000"])
def test_large_networks_decode_a_maximiser(host_engine, name):
    m = jr.networks()[name]
    ev = jr.hard_evidence(m, 0.1, 3)
    states, mm, _, lg = _restate(host_engine, m).run_max(ev)
    want = ev.hard_states(m)
    assert np.array_equal(states[want >= 0], want[want >= 0])
    jm.check_large(m, ev, states, mm, lg)


def test_contradictory_evidence(host_engine):
    m = synth.pearl()
    rs = _restate(host_engine, m)
    # R = 0 and W = 1: P(W = 1 | R = 0) = 0; and an all-zero vector
    for ev in (Evidence.from_dict(m, {0: 0, 2: 1}), Evidence.from_dict(m, {3: np.zeros(int(m.k[3]))})):
        states, mm, scales, lg = rs.run_max(ev)
        assert lg == -np.inf and np.isnan(mm).all() and (scales == 0).any()
        assert states.shape == (m.n,) and ((states >= 0) & (states < m.k)).all()   # defined, and meaningless


def test_errors_on_a_host_only_engine(host_engine):
    m = synth.pearl()
    L = _lib.lib()
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))   # noqa: E731
    mm, st = np.zeros(int(m.k.sum())), np.zeros(m.n, np.int32)
    lg = ctypes.c_double(0.0)
    with host_engine(m) as e:
        node, off, val = np.asarray([9], np.int32), np.asarray([0, 2], np.int32), np.asarray([1.0, 0.0])
        args = lambda a, b: (e._h, 1, p(node, ctypes.c_int32), p(off, ctypes.c_int32), p(val, ctypes.c_double), a, b, ctypes.byref(lg))   # noqa: E731
        assert L.bn_jt_mpe_run(*args(p(mm, ctypes.c_double), p(st, ctypes.c_int32))) == _lib.BN_ERR_ARG and b"out of range" in L.bn_last_error()
        node[0] = 3
        assert L.bn_jt_mpe_run(*args(None, p(st, ctypes.c_int32))) == _lib.BN_ERR_ARG and b"max_marginals_out" in L.bn_last_error()
        assert L.bn_jt_mpe_run(*args(p(mm, ctypes.c_double), None)) == _lib.BN_ERR_ARG and b"states_out" in L.bn_last_error()
        assert L.bn_jt_mpe_run(*args(p(mm, ctypes.c_double), p(st, ctypes.c_int32))) == _lib.BN_ERR_NO_DEVICE
        assert b"BN_DEVICE_HOST_ONLY" in L.bn_last_error()
        assert e.info("jt_last_kind") == 0 and L.bn_jt_scales(e._h, 0, p(mm, ctypes.c_double), 1) == _lib.BN_ERR_STATE
        with pytest.raises(_lib.BnError) as err:
            e.jt_mpe_run_batch([None, None])
        assert err.value.code == _lib.BN_ERR_NO_DEVICE
    with host_engine(synth.grid(8, 8, 4, seed=1)) as e:   # the plan's refusal comes before the missing device
        with pytest.raises(_lib.BnError) as err:
            e.jt_mpe_run()
        assert err.value.code == _lib.BN_ERR_STATE and "elimination clique" in str(err.value)
