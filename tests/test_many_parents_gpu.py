"""The item kernels on nodes with five to eight parents (the networks of tests/many_parents.py): a wave whose largest parent count is
5 or 6 runs the MM = 6 instantiation of item_entry (bn_small_dev.hpp: the one entry routine of all five kernels), 7 or 8 the MM = 8
one -- parent terms from LDS on every sweep, and a lane with
fewer parents than MM loads element 0 of the pi-message array for each missing factor and takes 1.0 instead.  Sum-product in one
workgroup (bn_small.hip) and in several (bn_mid.hip) against the oracle, max-product in both forms (bn_maxprod.hip) against
tests/maxprod_refs.py, EM (bn_em.hip) against tests/em_refs.py: all BIT FOR BIT -- beliefs, sweep counts, residual histories, both
message arrays.  The canary networks make element 0 a NaN: a padded factor that let the loaded value through would spoil the fan.
What the plans of these networks hold (which counts head a wave, at how many rounds) is pinned by tests/test_many_parents_refs.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import many_parents as mp  # noqa: E402
import maxprod_refs  # noqa: E402
from bayesiannetwork_amd import Evidence, synth  # noqa: E402
from test_em_gpu import check_against_restatement, random_table  # noqa: E402
from test_maxprod_gpu import check_form, evidences  # noqa: E402
from test_small_gpu import _same_as_oracle  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(bnlib):
    from bayesiannetwork_amd.engine import Engine
    return Engine


def _bp_cases(model, canary):
    """(name, evidence, eps, cap): none, 15 % and 30 % hard evidence, a soft vector with a zero on a many-parent child, a cap of 3;
    on a canary network the all-zero vector on node 0 as well"""
    cases = [("none", Evidence.none(), 1e-6, 0), ("hard15", synth.random_evidence(model, 0.15, seed=3), 1e-9, 0),
             ("hard30", synth.random_evidence(model, 0.3, seed=5), 1e-3, 0), ("soft_zero", mp.soft_zero(model), 1e-9, 0),
             ("cap3", synth.random_evidence(model, 0.15, seed=6), 1e-12, 3)]
    if canary:
        cases += [("canary", mp.canary_evidence(model), 1e-6, 0), ("canary_cap3", mp.canary_evidence(model), 1e-12, 3)]
    return cases


def _canary_holds(o):
    assert np.isnan(o["pi_msg"][0:3]).all() and np.isnan(o["beliefs"][:mp.CANARY_ELEMENTS]).all()
    assert np.isfinite(o["beliefs"][mp.CANARY_ELEMENTS:]).all()


# ---- sum-product, one workgroup ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(mp.SMALL) + list(mp.SMALL_CANARY))
def test_small_equals_oracle_bitwise(Engine, oracle_mod, name):
    model = {**mp.SMALL, **mp.SMALL_CANARY}[name]()
    with Engine(model) as eng:
        eng.set_option("small", 2)   # the one-workgroup path wherever eligible, whatever the policy would choose
        assert eng.info("small_eligible") == 1
        for what, ev, eps, cap in _bp_cases(model, name in mp.SMALL_CANARY):
            o = oracle_mod.bp_run(model, ev, eps, cap, dump_msgs=True)
            if what.startswith("canary"):
                _canary_holds(o)
            for rep in range(3):   # repeated runs: nothing of one run leaks into the next
                r = eng.bp_run(ev, eps, cap)
                assert eng.last_path() == 3 and eng.bp_stats()["sweep_launches"] == 1
                _same_as_oracle(r, eng.bp_residuals(), eng.bp_messages(), o)


def test_small_batch_equals_single_queries(Engine, oracle_mod):
    model = mp.SMALL["fan5678"]()
    sets = [synth.random_evidence(model, f, seed=20 + q) for q, f in enumerate([0.0, 0.15, 0.3, 0.1, 0.5, 0.2])] + [mp.soft_zero(model)]
    assert len(sets) == 7
    with Engine(model) as eng:
        eng.set_option("small", 2)
        singles = []
        for ev in sets:
            r = eng.bp_run(ev, 1e-9)
            assert eng.last_path() == 3
            singles.append((r, eng.bp_residuals()))
        for rep in range(3):
            out = eng.bp_run_batch(sets, 1e-9)
            assert eng.last_path() == 3 and eng.bp_stats()["sweep_launches"] == 1
            for q, ev in enumerate(sets):
                one, hist = singles[q]
                o = oracle_mod.bp_run(model, ev, 1e-9)
                assert out["sweeps"][q] == one["sweeps"] == o["sweeps"], q
                assert np.array_equal(out["beliefs"][q], one["beliefs"]) and np.array_equal(out["beliefs"][q], o["beliefs"]), q
                assert np.array_equal(eng.bp_residuals_batch(q), hist) and np.array_equal(hist, o["residuals"]), q
        assert len(set(out["sweeps"].tolist())) > 1   # the sets stop on sweeps of their own


# ---- sum-product, several workgroups -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(mp.MID) + list(mp.MID_CANARY))
def test_mid_equals_oracle_bitwise(Engine, oracle_mod, name):
    model = {**mp.MID, **mp.MID_CANARY}[name]()
    with Engine(model) as eng:
        eng.set_option("dag", 0)
        assert eng.info("small_eligible") == 0 and eng.info("mid_eligible") == 1 and eng.info("mid_parts") >= 2
        for what, ev, eps, cap in _bp_cases(model, name in mp.MID_CANARY):
            o = oracle_mod.bp_run(model, ev, eps, cap, dump_msgs=True)
            if what.startswith("canary"):
                _canary_holds(o)
            for rep in range(3):
                r = eng.bp_run(ev, eps, cap)
                assert eng.last_path() == 4 and eng.bp_stats()["sweep_launches"] == 1 and eng.info("mid_aborts") == 0
                _same_as_oracle(r, eng.bp_residuals(), eng.bp_messages(), o)


def test_mid_batch_equals_single_queries(Engine, oracle_mod):
    model = mp.MID["dag60_6parents_mixed"]()
    sets = [synth.random_evidence(model, f, seed=40 + q) for q, f in enumerate([0.0, 0.15, 0.3, 0.05])] + [mp.soft_zero(model)]
    assert len(sets) == 5
    with Engine(model) as eng:
        eng.set_option("dag", 0)
        singles = []
        for ev in sets:
            r = eng.bp_run(ev, 1e-9)
            assert eng.last_path() == 4
            singles.append((r, eng.bp_residuals()))
        for rep in range(3):
            out = eng.bp_run_batch(sets, 1e-9)
            assert eng.last_path() == 4 and eng.info("mid_aborts") == 0 and eng.info("mid_parts") >= 2
            for q, ev in enumerate(sets):
                one, hist = singles[q]
                o = oracle_mod.bp_run(model, ev, 1e-9)
                assert out["sweeps"][q] == one["sweeps"] == o["sweeps"], q
                assert np.array_equal(out["beliefs"][q], one["beliefs"]) and np.array_equal(out["beliefs"][q], o["beliefs"]), q
                assert np.array_equal(eng.bp_residuals_batch(q), hist) and np.array_equal(hist, o["residuals"]), q


# ---- max-product ---------------------------------------------------------------------------------------------------------------------

def _mpe_evidences(model, canary):
    """the evidence sets of tests/test_maxprod_gpu.py and a soft vector with a zero on a many-parent child; on a canary network none
    and the all-zero vector on node 0 (the restatement must show the NaN in element 0 and a finite fan)"""
    if not canary:
        return dict(evidences(model), soft_zero=mp.soft_zero(model))
    _canary_holds(maxprod_refs.run(model, mp.canary_evidence(model), 1e-9, 5))
    return {"none": None, "canary": mp.canary_evidence(model)}


MPE_SMALL = {**mp.SMALL, **mp.SMALL_CANARY}


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", list(MPE_SMALL))
def test_max_product_on_one_workgroup_networks(name, form):
    model = MPE_SMALL[name]()
    evs = _mpe_evidences(model, name in mp.SMALL_CANARY)
    parts = check_form(model, form, ev_names=tuple(evs), evs=evs)   # the settings, repeats and comparisons of tests/test_maxprod_gpu.py
    assert form == 1 or parts >= 3


MPE_MID = {**mp.MID, **mp.MID_CANARY}


@pytest.mark.parametrize("name", list(MPE_MID))
def test_max_product_on_several_workgroup_networks(name):
    model = MPE_MID[name]()
    evs = _mpe_evidences(model, name in mp.MID_CANARY)
    assert check_form(model, 2, ev_names=tuple(evs), evs=evs) >= 2


def test_max_product_forms_agree_bit_for_bit(Engine):
    model = mp.SMALL["fan5678"]()
    evs = evidences(model)
    with Engine(model, device=0) as eng:
        eng.set_option("mpe_form", 2)
        assert eng.info("mpe_form") == 2 and eng.info("mpe_parts") >= 2
        for name in ("none", "hard10", "soft", "zero"):
            eng.set_option("mpe_form", 1)
            a = eng.mpe_run(evs[name], 1e-9, 30)
            assert eng.info("mpe_last_form") == 1
            ra, ma = eng.mpe_residuals(0), eng.mpe_messages()
            eng.set_option("mpe_form", 2)
            b = eng.mpe_run(evs[name], 1e-9, 30)
            assert eng.info("mpe_last_form") == 2
            assert a["sweeps"] == b["sweeps"] and np.array_equal(a["states"], b["states"]), name
            assert np.array_equal(a["max_marginals"], b["max_marginals"], equal_nan=True), name
            assert np.array_equal(ra, eng.mpe_residuals(0)), name
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ma, eng.mpe_messages())), name


# ---- expectation-maximisation --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fan5", "fan7", "fan5678", "fan5_kp4", "fan7x6"])   # one, one, two, three and three rounds
def test_em_equals_the_restatement(Engine, name):
    model = mp.SMALL[name]()
    with Engine(model, device=0) as eng:
        plan = eng.small_plan()
        assert plan is not None and plan["mmax"] == mp.SMALL_PLAN[name][1] and plan["re"] == mp.SMALL_PLAN[name][0]
    pats, counts = random_table(model, 12, 0.25, seed=31)
    check_against_restatement(model, pats, counts, scratch_rows=10, what=name, bp_max_sweeps=12)
