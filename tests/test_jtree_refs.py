"""Junction-tree propagation on the CPU: the plan the library builds on a BN_DEVICE_HOST_ONLY engine has the properties a junction
tree must have, and the numpy restatement of the arithmetic over that plan (tests/jtree_refs.py) equals exact inference --
tests/exact_refs.py: einsum_marginals (long double, any small DAG, hard evidence) and exact_marginals(bp_clamp=False) (long
double, polytrees, hard and soft evidence) -- to 1e-12 absolute in the beliefs and 1e-12 relative in log P(e).  Also the argument
and state errors of bn_jt_run on an engine without a device."""
import ctypes

import numpy as np
import pytest

from bayesiannetwork_amd import Evidence, _lib, engine, synth

import exact_refs as xr
import jtree_refs as jr


@pytest.fixture(scope="module")
def host_engine(bnlib):
    return lambda m: engine.Engine(m, device=_lib.BN_DEVICE_HOST_ONLY)


@pytest.fixture(scope="module")
def nets():
    return jr.networks()


# the form every network must land in (None: whatever the plan gives): form 1 keeps a state of at most 8192 doubles in LDS
EXPECTED = {"pearl": 1, "alarm": 1, "arity7": 1, "grid3x8": None, "dag37": None, "star": 1, "wide12": 2, "grid8x8k2": 2, "grid4x40": 2,
            "chain3000": 2}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_plan_is_a_junction_tree(host_engine, nets, name):
    m = nets[name]
    with host_engine(m) as e:
        assert e.info("jt_eligible") == 1
        plan = e.jt_plan()
        jr.check_plan(m, plan)
        print(name, plan["cliques"], plan["max_clique"], plan["pot_cells"], "levels", plan["levels"], "form", plan["form"])
        assert EXPECTED[name] in (None, plan["form"])
        assert e.info("jt_cliques") == plan["cliques"] and e.info("jt_levels") == plan["levels"]
        assert e.info("jt_max_clique") == plan["max_clique"] and e.info("jt_state_cells") == plan["state_cells"]
        assert e.info("jt_form") == (1 if plan["state_cells"] <= 8192 else 2)


def test_grid8x8k4_is_refused_with_the_clique_named(host_engine):
    m = synth.grid(8, 8, 4, seed=1)
    with host_engine(m) as e:
        assert e.info("jt_eligible") == 0 and e.info("jt_form") == 0
        with pytest.raises(_lib.BnError) as err:
            e.jt_plan()
        assert err.value.code == _lib.BN_ERR_STATE
        msg = str(err.value)
        assert "elimination clique of node" in msg and "variables and" in msg and "above the limit of 1048576 entries" in msg
        size = int(msg.split("variables and ")[1].split(" entries")[0])
        assert size > 1 << 20


def test_scratch_budget_is_a_fact_of_the_plan(host_engine, nets):
    m = nets["grid3x8"]
    with host_engine(m) as e:
        cells = e.info("jt_state_cells")
        e.set_option("jt_scratch_cells", cells - 1)
        assert e.info("jt_eligible") == 0
        e.set_option("jt_scratch_cells", cells)
        assert e.info("jt_eligible") == 1
        e.set_option("jt_scratch_cells", 0)
        assert e.info("jt_scratch_cells") == 1 << 22
    with host_engine(m) as e:   # the budget set before the plan exists: the plan stops there, and is built again once it fits
        e.set_option("jt_scratch_cells", 100)
        assert e.info("jt_eligible") == 0
        e.set_option("jt_scratch_cells", 0)
        assert e.info("jt_eligible") == 1
        jr.check_plan(m, e.jt_plan())


def _restate(host_engine, m):
    with host_engine(m) as e:
        return jr.Restatement(m, e.jt_plan())


EINSUM = {"pearl": lambda: synth.pearl(), "alarm": jr.alarm, "grid3x3": lambda: synth.grid(3, 3, 4, seed=1),
          "grid3x8": lambda: synth.grid(3, 8, 4, seed=1), "grid4x4k3": lambda: synth.grid(4, 4, 3, seed=1),
          "dag37": lambda: synth.random_dag(37, 3, 4, jr.MIXED, seed=5)}


@pytest.mark.parametrize("name", sorted(EINSUM))
def test_restatement_equals_einsum_elimination(host_engine, name):
    m = EINSUM[name]()
    rs = _restate(host_engine, m)
    for ev in (None, jr.hard_evidence(m, 0.1, 3), jr.hard_evidence(m, 0.3, 4)):
        joint, pe = xr.einsum_marginals(m, None if ev is None else jr.ev_state_of(m, ev))
        bel, scales, lg = rs.run(ev)
        off = m.node_off
        want = np.concatenate([joint[off[v]:off[v + 1]] / pe for v in range(m.n)])
        dev = float(np.abs(bel - want).max())
        print(name, "evidence", 0 if ev is None else ev.ne, "belief deviation", dev, "log P(e)", lg, np.log(pe))
        assert dev <= 1e-12
        assert abs(lg - np.log(pe)) <= 1e-12 * max(1.0, abs(np.log(pe)))
        assert abs(np.prod(scales) - pe) <= 1e-12 * pe


def _polytrees():
    z = xr.polytree(300, (2, 3, 4), 3, 4, zero_frac=0.3, seed=5, name="zeros")
    s = xr.star(120, 3, 5, seed=1)
    w = xr.wide(12, seed=12)
    c = xr.chain(3000, 3, seed=1)
    return {"zeros": (z, [xr.draw_evidence(z, 20, seed=4, soft=0.5), xr.draw_evidence(z, 30, seed=5)]),
            "star": (s, [xr.draw_evidence(s, 10, seed=6, soft=0.3), xr.draw_evidence(s, 12, seed=7)]),
            "wide12": (w, [xr.draw_evidence(w, 2, seed=12, soft=0.5), xr.draw_evidence(w, 3, seed=13)]),
            "chain3000": (c, [xr.draw_evidence(c, 6, seed=5, soft=0.5), xr.draw_evidence(c, 300, seed=6)])}


@pytest.mark.parametrize("name", ["zeros", "star", "wide12", "chain3000"])
def test_restatement_equals_two_pass_sum_product_on_polytrees(host_engine, name):
    m, evs = _polytrees()[name]
    rs = _restate(host_engine, m)
    for ev in [None] + evs:
        want, logz = xr.exact_marginals(m, ev, bp_clamp=False)
        bel, _, lg = rs.run(ev)
        dev = float(np.abs(bel - want).max())
        print(name, "evidence", 0 if ev is None else ev.ne, "belief deviation", dev, "log P(e)", lg, logz)
        assert dev <= 1e-12
        assert abs(lg - logz) <= 1e-12 * max(1.0, abs(logz))


def test_impossible_and_all_zero_evidence(host_engine):
    m = synth.pearl()
    rs = _restate(host_engine, m)
    bel, scales, lg = rs.run(Evidence.from_dict(m, {3: np.zeros(int(m.k[3]))}))
    assert np.isnan(bel).all() and lg == -np.inf and (scales == 0).any()


def test_errors_on_a_host_only_engine(host_engine):
    m = synth.pearl()
    L = _lib.lib()
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))   # noqa: E731
    bel = np.zeros(int(m.k.sum()))
    lg = ctypes.c_double(0.0)
    with host_engine(m) as e:
        node, off, val = np.asarray([9], np.int32), np.asarray([0, 2], np.int32), np.asarray([1.0, 0.0])
        rc = L.bn_jt_run(e._h, 1, p(node, ctypes.c_int32), p(off, ctypes.c_int32), p(val, ctypes.c_double), p(bel, ctypes.c_double), ctypes.byref(lg))
        assert rc == _lib.BN_ERR_ARG and b"out of range" in L.bn_last_error()
        node[0] = 3
        rc = L.bn_jt_run(e._h, 1, p(node, ctypes.c_int32), p(off, ctypes.c_int32), p(val, ctypes.c_double), None, ctypes.byref(lg))
        assert rc == _lib.BN_ERR_ARG
        rc = L.bn_jt_run(e._h, 1, p(node, ctypes.c_int32), p(off, ctypes.c_int32), p(val, ctypes.c_double), p(bel, ctypes.c_double), ctypes.byref(lg))
        assert rc == _lib.BN_ERR_NO_DEVICE and b"BN_DEVICE_HOST_ONLY" in L.bn_last_error()
        assert L.bn_jt_scales(e._h, 0, p(bel, ctypes.c_double), 1) == _lib.BN_ERR_STATE
        with pytest.raises(_lib.BnError):
            e.set_option("jt_form", 3)
        e.set_option("jt_form", 2)
        assert e.info("jt_form") == 2 and e.info("jt_last_form") == 0
    with host_engine(synth.grid(8, 8, 4, seed=1)) as e:   # the plan's refusal comes before the missing device
        with pytest.raises(_lib.BnError) as err:
            e.jt_run()
        assert err.value.code == _lib.BN_ERR_STATE and "elimination clique" in str(err.value)
