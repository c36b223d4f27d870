"""Nodes with five to eight parents on the item kernels' plans, without a GPU: the facts of the plans the networks of
tests/many_parents.py get from a host-only engine (path eligibility, rounds, largest parent count, waves, parts), the plans executed
on the CPU (tests/small_emulator.py) against the oracle bit for bit, the canary that makes element 0 of the pi-message array a NaN
and must leave the fan's beliefs finite, and the coverage tests/test_many_parents_gpu.py relies on: which parent counts head a wave,
at how many rounds, next to which smaller counts.

A several-workgroup part with two rounds of entry items AND a largest parent count of 7 or 8 was searched for over seeds 1..20:
binary networks (random_dag(40, 8, 20, 2), random_dag(60, 8, 16, 2)) have none -- an 8-parent binary table is 512 entries, one round
-- and random_dag(60, 8, 16, [2, 3, 2, 2, 3]) is beyond the path at every seed; random_dag(40, 8, 20, [2, 2, 3]) has such parts at
seeds 5, 7 and 11.  Seed 5 is MID["dag40_8parents_k223"]: one part of two rounds at 7 parents and one at 8, a node each.

Not reachable: three rounds at 8 parents.  A third round needs more than 1 536 entry items in a workgroup (12 waves), an 8-parent
entry stages 9 doubles and 8 term words, 104 bytes: 160 KB, beyond the 150 KB of LDS the plans may use (bn_small.hpp kSmallLdsBytes).
At 7 parents (92 bytes) it fits: SMALL["fan7x6"].  Not looked for beyond the seeds above, and not among the networks here: a
several-workgroup part of three rounds at five or more parents (a part goes to 16 waves first: more than 2 048 entries, 136 KB at 5)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import many_parents as mp  # noqa: E402
import small_emulator  # noqa: E402
from bayesiannetwork_amd import Evidence, synth  # noqa: E402


@pytest.fixture(scope="module")
def E(bnlib):
    from bayesiannetwork_amd import _lib, engine
    return lambda m, **kw: engine.Engine(m, device=_lib.BN_DEVICE_HOST_ONLY, **kw)


@pytest.fixture(scope="module")
def small_plans(E):
    out = {}
    for name, make in {**mp.SMALL, **mp.SMALL_CANARY}.items():
        model = make()
        with E(model) as e:
            assert e.info("small_eligible") == 1, name
            out[name] = (model, e.small_plan())
    return out


@pytest.fixture(scope="module")
def mid_plans(E):
    out = {}
    for name, make in {**mp.MID, **mp.MID_CANARY}.items():
        model = make()
        with E(model) as e:
            assert e.info("small_eligible") == 0 and e.info("mid_eligible") == 1, name
            out[name] = (model, e.mid_plan())
    return out


def test_waves_of_reads_flag_and_count():
    ent = np.zeros((128, 2), dtype=np.uint32)
    ent[0, 1] = (1 << 24) | (5 << 16) | 77
    ent[1, 1] = (1 << 24) | (0 << 16)
    ent[2, 1] = (0 << 24) | (8 << 16)        # not valid: its count is not the wave's
    ent[3, 1] = (1 << 24) | (5 << 16) | 3
    assert mp.waves_of({"ent": ent}) == [[0, 5], []]
    assert mp.top_counts({"ent": ent}) == [5] and mp.padded_mixed_waves({"ent": ent}) == [[0, 5]]


@pytest.mark.parametrize("name", list(mp.SMALL))
def test_small_plan_facts(E, small_plans, name):
    model, plan = small_plans[name]
    re_, mmax, waves = mp.SMALL_PLAN[name]
    assert (plan["re"], plan["mmax"]) == (re_, mmax)
    assert int(np.diff(model.in_ptr).max()) == mmax == max(mp.top_counts(plan))
    if waves is not None:
        assert plan["waves"] == waves
    if name in ("fan5", "fan6", "fan7", "fan8"):
        assert plan["rb"] == 1 and plan["rc"] == 1
    if name == "fan5_kp3":
        v = mp.many_parent_child(model)
        assert int(model.cpt_off[v + 1] - model.cpt_off[v]) == 486
        # 243-term runs of pi(v) and 162-term runs of the lambda-messages, padded to a multiple of 4
        assert {164, 244} <= set((plan["bslot"][:, 0] >> 16).tolist())
    if name.startswith("fan") and name not in ("fan5_kc3", "fan5_kp3"):   # a many-parent wave holds one parent count
        assert all(len(w) == 1 or w[-1] <= 1 for w in mp.waves_of(plan) if w)
    with E(model) as e:
        assert e.info("em_eligible") == 1
        assert e.info("mpe_form") == 1
        e.set_option("mpe_form", 2)
        assert e.info("mpe_form") == 2 and 3 <= e.info("mpe_parts") <= 8


@pytest.mark.parametrize("name", list(mp.MID))
def test_mid_plan_facts(E, mid_plans, name):
    model, parts = mid_plans[name]
    assert len(parts) == mp.MID_PARTS[name]
    assert parts[0]["v0"] == 0 and parts[-1]["v1"] == model.n and all(a["v1"] == b["v0"] for a, b in zip(parts, parts[1:]))
    mmax = [p["mmax"] for p in parts]
    if name == "fan8x4":
        assert max(mmax) == 8
    if name == "dag40_8parents":
        assert min(mmax) == 3 and max(mmax) == 8 and all(p["re"] == 1 for p in parts)
    if name == "dag60_6parents_mixed":
        assert [(p["re"], p["mmax"]) for p in parts if p["re"] >= 2] == [(2, 6)]
        mixed = [w for p in parts for w in mp.waves_of(p)]
        assert [0, 1, 3, 5] in mixed and [1, 3, 5] in mixed and [4, 5] in mixed
    if name == "dag40_8parents_k223":
        assert sorted((p["re"], p["mmax"]) for p in parts if p["re"] >= 2 and p["mmax"] >= 7) == [(2, 7), (2, 8)]
    with E(model) as e:
        assert e.info("mpe_form") == 2 and e.info("mpe_parts") == len(parts)


def _settings(model):
    return [(Evidence.none(), 1e-6, 0), (synth.random_evidence(model, 0.15, seed=3), 1e-9, 0), (synth.random_evidence(model, 0.15, seed=5), 1e-12, 3)]


def _emulated_equals_oracle(oracle_mod, model, plan, ev, eps, cap, what):
    got = small_emulator.emulate(plan, model, ev, eps, cap)
    want = oracle_mod.bp_run(model, ev, eps, cap, dump_msgs=True)
    assert got["sweeps"] == want["sweeps"], what
    assert np.array_equal(got["beliefs"], want["beliefs"], equal_nan=True), what
    assert np.array_equal(got["residuals"], want["residuals"]), what
    assert np.array_equal(got["pi_msg"], want["pi_msg"], equal_nan=True), what
    assert np.array_equal(got["lambda_msg"], want["lambda_msg"], equal_nan=True), what
    return want


@pytest.mark.parametrize("name", list(mp.SMALL))
def test_small_plan_emulated_equals_oracle(oracle_mod, small_plans, name):
    model, plan = small_plans[name]
    for ev, eps, cap in _settings(model) + [(mp.soft_zero(model), 1e-9, 0)]:
        want = _emulated_equals_oracle(oracle_mod, model, plan, ev, eps, cap, (name, eps, cap))
        assert np.isfinite(want["beliefs"]).all()
        assert cap == 0 or want["sweeps"] == cap


@pytest.mark.parametrize("name", list(mp.MID))
def test_mid_plan_emulated_equals_oracle(oracle_mod, mid_plans, name):
    model, parts = mid_plans[name]
    for ev, eps, cap in _settings(model):
        _emulated_equals_oracle(oracle_mod, model, parts, ev, eps, cap, (name, eps, cap))


@pytest.mark.parametrize("name", list(mp.SMALL_CANARY) + list(mp.MID_CANARY))
def test_canary_spoils_element_zero_and_nothing_of_the_fan(oracle_mod, small_plans, mid_plans, name):
    model, plan = small_plans[name] if name in small_plans else mid_plans[name]
    assert int(model.in_idx[0]) == 0 and int(model.in_ptr[1]) == 0 and int(model.in_ptr[2]) == 1   # edge 0 is node 0 -> node 1
    want = _emulated_equals_oracle(oracle_mod, model, plan, mp.canary_evidence(model), 1e-6, 0, name)
    assert np.isnan(want["pi_msg"][0:3]).all() and np.isfinite(want["pi_msg"][3:]).all()
    assert np.isnan(want["beliefs"][:mp.CANARY_ELEMENTS]).all() and np.isfinite(want["beliefs"][mp.CANARY_ELEMENTS:]).all()
    # ... and the padded lanes are there to load it: waves of the fan run at 5 or 7 parents (at 8 no lane pads)
    assert (name == "canary_fan8x4") != bool({5, 7} & set(mp.top_counts(plan)))


def test_maxprod_restatement_sees_the_canary_too():
    import maxprod_refs
    for name, make in mp.SMALL_CANARY.items():
        model = make()
        want = maxprod_refs.run(model, mp.canary_evidence(model), 1e-6, 20)
        assert np.isnan(want["pi_msg"][0:3]).all() and np.isfinite(want["pi_msg"][3:]).all(), name
        assert np.isnan(want["beliefs"][:mp.CANARY_ELEMENTS]).all() and np.isfinite(want["beliefs"][mp.CANARY_ELEMENTS:]).all(), name


def test_coverage_the_gpu_tests_rely_on(small_plans, mid_plans):
    small = {n: p for n, (_, p) in small_plans.items()}
    mid = {n: p for n, (_, p) in mid_plans.items()}
    # every count from 5 to 8 heads a wave, on both paths
    assert {5, 6, 7, 8} <= {c for p in small.values() for c in mp.top_counts(p)}
    assert {5, 6, 7, 8} <= {c for p in mid.values() for c in mp.top_counts(p)}
    # two rounds of entry items: at MM = 8 in one workgroup, at MM = 6 in a part of several
    assert any(p["re"] >= 2 and p["mmax"] >= 7 for p in small.values())
    assert any(q["re"] >= 2 and q["mmax"] in (5, 6) for p in mid.values() for q in p)
    assert any(q["re"] >= 2 and q["mmax"] >= 7 for p in mid.values() for q in p)
    # three rounds (the kernels' four-round instantiation) in one workgroup: at MM = 6 and at MM = 8
    assert small["fan5_kp4"]["re"] == 3 and set(mp.top_counts(small["fan5_kp4"])) == {1, 5}
    assert small["fan7x6"]["re"] == 3 and set(mp.top_counts(small["fan7x6"])) == {1, 7}
    # ... and in both rounds a wave runs padded there (the second round's waves are the plan's last ones)
    for name in ("fan5678", "dag20_8parents", "dag26_8parents"):
        p = small[name]
        waves = mp.waves_of(p)
        assert len(waves) == p["re"] * p["waves"]
        assert all(any(w and w[-1] >= 5 for w in waves[r * p["waves"]:(r + 1) * p["waves"]]) for r in range(p["re"])), name
    # a wave at 5 or 7 parents (every lane pads) that also holds lanes with fewer parents (they pad more than one factor)
    assert mp.padded_mixed_waves(mid["dag60_6parents_mixed"])
    assert mp.padded_mixed_waves(small["fan5_kc3"]) == [[0, 1, 5]]   # the 5-parent node's last 32 entries, the roots' and the leaf's
    assert mp.padded_mixed_waves(small["fan5_kp3"]) == [[0, 1, 5]]
    assert not any(mp.padded_mixed_waves(small[n]) for n in ("dag20_8parents", "dag26_8parents"))   # (sorted by count: waves of one count)
    # the fans' waves are homogeneous: a wave of the 5-parent node pads exactly one factor in every lane, and so one of the 7-parent node
    for name, count in (("fan5", 5), ("fan7", 7), ("canary_fan5", 5), ("canary_fan7", 7)):
        assert [count] in mp.waves_of(small[name]), name
    assert all(c in mp.top_counts(small["fan5678"]) for c in (5, 6, 7, 8))


def test_search_for_a_mid_part_of_two_rounds_at_seven_parents(E):
    """the search the module docstring reports, seeds 1..20 of each shape: parts with re >= 2 and mmax >= 7"""
    def seeds_with_such_a_part(make):
        hits = []
        for seed in range(1, 21):
            with E(make(seed)) as e:
                if e.info("mid_eligible") == 1 and e.info("small_eligible") == 0 and any(p["re"] >= 2 and p["mmax"] >= 7 for p in e.mid_plan()):
                    hits.append(seed)
        return hits
    assert seeds_with_such_a_part(lambda s: synth.random_dag(40, 8, 20, 2, seed=s)) == []
    assert seeds_with_such_a_part(lambda s: synth.random_dag(40, 8, 20, [2, 2, 3], seed=s)) == [5, 7, 11]
