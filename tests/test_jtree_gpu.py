"""Junction-tree propagation on the GPU (bn_jt_* of include/bn_mi355x.h; Engine.jt_run / jt_run_batch, JunctionTree) against the
numpy restatement tests/jtree_refs.py: beliefs and scale arrays BIT FOR BIT (NaNs as NaNs), log P(e) to 1e-12 relative (numpy's
and the C library's log may differ in the last place).  Both forms, every evidence kind three times in a row, batches whose sets
must have the bits of their single queries, a form-2 batch cut into three launches, the calls around a run, bn_reload_cpt, and
the refusals."""
import numpy as np
import pytest

from bayesiannetwork_amd import Evidence, FlatModel, _lib, from_parent_lists, synth
from bayesiannetwork_amd.engine import Engine, JunctionTree

import exact_refs as xr
import jtree_refs as jr

pytestmark = pytest.mark.gpu


def _lone_root():
    return from_parent_lists([3], [[]], [np.asarray([0.2, 0.5, 0.3])], name="lone")


def _two_roots():
    return from_parent_lists([2, 3], [[], []], [np.asarray([0.25, 0.75]), np.asarray([0.2, 0.5, 0.3])], name="two")


FORM1 = {"lone": _lone_root, "two": _two_roots, "pearl": synth.pearl, "resume_chain": synth.resume_chain, "alarm": jr.alarm,
         "arity7": lambda: synth.random_dag(16, 2, 8, [7, 5, 6, 2], seed=8),
         "mixed12": lambda: synth.random_dag(12, 3, 16, jr.MIXED, seed=2),
         "star": lambda: xr.star(120, 3, 5), "grid3x3": lambda: synth.grid(3, 3, 4, seed=1)}
ANY = {"grid3x8": lambda: synth.grid(3, 8, 4, seed=1), "dag37": lambda: synth.random_dag(37, 4, 16, jr.MIXED, seed=5)}
FORM2 = {"wide12": lambda: xr.wide(12), "grid8x8k2": lambda: synth.grid(8, 8, 2, seed=1), "grid4x40": lambda: synth.grid(4, 40, 4, seed=1),
         "chain3000": lambda: xr.chain(3000, 3)}


def evidence_kinds(m):
    """none; 10 % and 30 % hard; a soft vector with a zero in it; an all-zero vector (P(e) = 0)."""
    rng = np.random.default_rng(m.n)
    v = m.n // 2
    soft = 0.05 + rng.random(int(m.k[v]))
    soft[0] = 0.0
    return [("none", None), ("hard10", jr.hard_evidence(m, 0.1, 3)), ("hard30", jr.hard_evidence(m, 0.3, 4)),
            ("soft0", Evidence.from_dict(m, {v: soft, (v + 1) % m.n: 0.05 + rng.random(int(m.k[(v + 1) % m.n]))} if m.n > 1 else {v: soft})),
            ("zero", Evidence.from_dict(m, {v: np.zeros(int(m.k[v]))}))]


def same_log(a, b, scales):
    """log P(e) is a sum of logarithms that may cancel (no evidence: log 3 + log 1/3 + ... = 0), and numpy's and the C library's
    log may differ in the last place of every TERM: 1e-12 relative to the sum of the terms' magnitudes.  (-inf == -inf.)"""
    with np.errstate(divide="ignore"):
        terms = np.abs(np.log(scales))
    return a == b or abs(a - b) <= 1e-12 * float(terms[np.isfinite(terms)].sum())


def check_run(got, want, what):
    bel, scales, lg = want
    assert jr.same_bits(got["beliefs"], bel), (what, "beliefs", float(np.nanmax(np.abs(got["beliefs"] - bel))))
    assert jr.same_bits(got["scales"], scales), (what, "scales")
    assert same_log(got["log_evidence"], lg, scales), (what, got["log_evidence"], lg)


def run_kinds(m, form, three=True):
    with Engine(m, device=0) as e:
        if form:
            assert e.info("jt_form") == form
        rs = jr.Restatement(m, e.jt_plan())
        for name, ev in evidence_kinds(m):
            want = rs.run(ev)
            for rep in range(3 if three else 1):
                check_run(e.jt_run(ev), want, (m.name, name, rep))
            assert e.info("jt_last_form") == (form or e.info("jt_form"))
            if name == "zero":   # P(e) = 0: -inf, and NaN beliefs -- in the zero node's tree (the trees of a forest normalise apart)
                v, off, plan = m.n // 2, m.node_off, e.jt_plan()
                assert want[2] == -np.inf and np.isnan(want[0][off[v]:off[v + 1]]).all()
                assert np.isnan(want[0]).all() or int((plan["parent"] < 0).sum()) > 1
            elif name != "soft0":
                assert np.isfinite(want[0]).all() and abs(want[0].sum() - m.n) < 1e-9


@pytest.mark.parametrize("name", sorted(FORM1))
def test_form1_equals_the_restatement(bnlib, name):
    run_kinds(FORM1[name](), 1)


@pytest.mark.parametrize("name", sorted(ANY))
def test_whatever_form_equals_the_restatement(bnlib, name):
    run_kinds(ANY[name](), 0)


@pytest.mark.parametrize("name", sorted(FORM2))
def test_form2_equals_the_restatement(bnlib, name):
    run_kinds(FORM2[name](), 2, three=name != "chain3000")


def test_chain3000_three_runs_in_a_row(bnlib):
    m = FORM2["chain3000"]()
    ev = xr.draw_evidence(m, 300, seed=6, soft=0.3)
    with Engine(m, device=0) as e:
        want = jr.Restatement(m, e.jt_plan()).run(ev)
        for rep in range(3):
            check_run(e.jt_run(ev), want, ("chain3000", rep))
        assert e.info("jt_last_form") == 2 and np.isfinite(want[2])


def test_forced_form2_has_the_bits_of_form1(bnlib):
    m = jr.alarm()
    with Engine(m, device=0) as e1, Engine(m, device=0) as e2:
        e2.set_option("jt_form", 2)
        for name, ev in evidence_kinds(m):
            a, b = e1.jt_run(ev), e2.jt_run(ev)
            assert e1.info("jt_last_form") == 1 and e2.info("jt_last_form") == 2
            assert jr.same_bits(a["beliefs"], b["beliefs"]) and jr.same_bits(a["scales"], b["scales"]), name
            assert a["log_evidence"] == b["log_evidence"] or (np.isnan(a["log_evidence"]) and np.isnan(b["log_evidence"]))


def test_impossible_hard_evidence(bnlib):
    """Hard evidence that a zero CPT entry makes impossible -- a node at a state its parents' states exclude: P(e) = 0, NaN beliefs
    (in that node's tree of the forest), -inf."""
    m = xr.polytree(300, (2, 3, 4), 3, 4, zero_frac=0.3, seed=5, name="zeros")
    v = next(v for v in range(m.n) if len(m.parents(v)) >= 2 and (m.cpt_of(v) == 0.0).any())
    row, x = [int(i) for i in np.argwhere(m.cpt_of(v) == 0.0)[0]]
    states = {v: x}
    for u in reversed([int(u) for u in m.parents(v)]):   # first parent most significant
        states[u] = row % int(m.k[u])
        row //= int(m.k[u])
    ev = Evidence.from_dict(m, states)
    off = m.node_off
    with Engine(m, device=0) as e:
        rs = jr.Restatement(m, e.jt_plan())
        want = rs.run(ev)
        assert want[2] == -np.inf and np.isnan(want[0][off[v]:off[v + 1]]).all()
        for rep in range(3):
            check_run(e.jt_run(ev), want, ("zeros", rep))
        ok = xr.draw_evidence(m, 30, seed=5)
        want = rs.run(ok)
        assert np.isfinite(want[0]).all() and np.isfinite(want[2])
        check_run(e.jt_run(ok), want, "zeros, possible")


@pytest.fixture(scope="module")
def alarm_singles(bnlib):
    m = jr.alarm()
    evs = [None] + [jr.hard_evidence(m, f, s) for f, s in ((0.1, 3), (0.3, 4), (0.2, 5), (0.1, 6), (0.3, 7))] + [e for _, e in evidence_kinds(m)[3:]]
    with Engine(m, device=0) as e:
        rs = jr.Restatement(m, e.jt_plan())
        singles = [e.jt_run(ev) for ev in evs]
        for ev, s in zip(evs, singles):
            check_run(s, rs.run(ev), "single")
    return m, evs, singles


@pytest.mark.parametrize("n_sets", [1, 3, 64, 600])
def test_batch_sets_have_the_bits_of_their_single_queries(alarm_singles, n_sets):
    m, evs, singles = alarm_singles
    pick = [(5 * q + q // 7) % len(evs) for q in range(n_sets)]
    with Engine(m, device=0) as e:
        got = e.jt_run_batch([evs[i] for i in pick])
        assert e.info("jt_last_form") == 1 and e.info("jt_last_launches") == 1
    for q, i in enumerate(pick):
        assert jr.same_bits(got["beliefs"][q], singles[i]["beliefs"]) and jr.same_bits(got["scales"][q], singles[i]["scales"]), q
        assert got["log_evidence"][q] == singles[i]["log_evidence"]


def test_form2_batch_cut_into_three_launches(bnlib):
    m = FORM2["grid8x8k2"]()
    evs = [None, jr.hard_evidence(m, 0.1, 3), jr.hard_evidence(m, 0.3, 4), evidence_kinds(m)[3][1], jr.hard_evidence(m, 0.2, 5)]
    with Engine(m, device=0) as e:
        singles = [e.jt_run(ev) for ev in evs]
        e.set_option("jt_scratch_cells", 2 * e.info("jt_state_cells") + 5)   # two sets per launch
        got = e.jt_run_batch(evs)
        assert e.info("jt_last_form") == 2 and e.info("jt_last_launches") == 3
        rs = jr.Restatement(m, e.jt_plan())
    for q, s in enumerate(singles):
        assert jr.same_bits(got["beliefs"][q], s["beliefs"]) and jr.same_bits(got["scales"][q], s["scales"]), q
        assert got["log_evidence"][q] == s["log_evidence"]
    check_run(singles[2], rs.run(evs[2]), "grid8x8k2 hard30")


def test_jt_run_between_the_other_calls(bnlib):
    """bp_run, bp_run_device, bp_messages, mpe_run, em_expected_counts with and without jt_run calls between them: the same results."""
    m = jr.alarm()
    ev, ev2, ev3 = synth.random_evidence(m, 0.1, seed=7), synth.random_evidence(m, 0.3, seed=11), jr.hard_evidence(m, 0.2, 9)
    rng = np.random.default_rng(3)
    pats = np.stack([xr.forward_sample(m, rng) for _ in range(12)]).astype(np.uint8)
    pats[rng.random(pats.shape) < 0.25] = 255
    counts = np.ones(12, dtype=np.uint64)

    def sequence(e, jt):
        out = []
        r = e.bp_run(ev, 1e-6); out += [r["beliefs"].copy(), r["sweeps"], e.last_path()]
        jt(e)
        e.bp_set_evidence(ev2)
        jt(e)
        r = e.bp_run_device(1e-6); out += [e.bp_beliefs(), r["sweeps"], r["residual"]]
        jt(e)
        out += list(e.bp_messages()) + [e.bp_residuals(), e.last_path()]
        r = e.mpe_run(ev2, 1e-6, 40); out += [r["states"], r["max_marginals"], r["sweeps"]]
        jt(e)
        out += list(e.mpe_messages())
        E, sw = e.em_expected_counts(pats, counts, 1e-6, 40); out += [E, sw]
        jt(e)
        r = e.bp_run_device(1e-6); out += [e.bp_beliefs(), r["sweeps"]]   # the evidence in force is still ev2
        return out

    with Engine(m, device=0) as plain, Engine(m, device=0) as mixed:
        a = sequence(plain, lambda e: None)
        b = sequence(mixed, lambda e: (e.jt_run(ev3), e.jt_run_batch([ev, None, ev3])))
        want = jr.Restatement(m, mixed.jt_plan()).run(ev3)
        check_run(mixed.jt_run(ev3), want, "after the others")
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), i


def test_reload_cpt_reaches_the_potentials(bnlib):
    m = jr.alarm()
    rng = np.random.default_rng(5)
    cpt = m.cpt.copy()
    for v in range(m.n):
        t = cpt[m.cpt_off[v]:m.cpt_off[v + 1]].reshape(-1, int(m.k[v]))
        t *= 0.2 + rng.random(t.shape)
        t /= t.sum(axis=1, keepdims=True)
    ev = jr.hard_evidence(m, 0.2, 3)
    with Engine(m, device=0) as e:
        plan = e.jt_plan()
        before = e.jt_run(ev)
        check_run(before, jr.Restatement(m, plan).run(ev), "old tables")
        e.reload_cpt(cpt)
        after = e.jt_run(ev)
        m2 = FlatModel(m.k, m.in_ptr, m.in_idx, m.cpt_off, cpt, name="alarm_edited")
        check_run(after, jr.Restatement(m2, plan).run(ev), "new tables")
        assert not np.array_equal(before["beliefs"], after["beliefs"])


def test_refusals(bnlib):
    with Engine(synth.grid(8, 8, 4, seed=1), device=0) as e:
        with pytest.raises(_lib.BnError) as err:
            e.jt_run()
        assert err.value.code == _lib.BN_ERR_STATE and "elimination clique of node" in str(err.value) and "above the limit of 1048576" in str(err.value)
    with Engine(FORM2["grid4x40"](), device=0) as e:
        e.set_option("jt_form", 1)
        assert e.info("jt_form") == 0
        with pytest.raises(_lib.BnError) as err:
            e.jt_run()
        assert err.value.code == _lib.BN_ERR_STATE and "option jt_form = 1" in str(err.value)
    with Engine(synth.grid(12, 12, 4, seed=2), device=0, rank=0, nranks=2) as shard:
        assert shard.info("jt_eligible") == 0
        with pytest.raises(_lib.BnError) as err:
            shard.jt_run()
        assert err.value.code == _lib.BN_ERR_STATE and "not available on sharded engines" in str(err.value)


def test_junction_tree_class(bnlib):
    m = synth.pearl()
    jt = JunctionTree(m, device=0)
    try:
        marg = jt({3: 0})
        joint, pe = xr.einsum_marginals(m, np.asarray([-1, -1, -1, 0, -1][:m.n]))
        off = m.node_off
        for v in range(m.n):
            assert np.abs(marg[v] - joint[off[v]:off[v + 1]] / pe).max() <= 1e-12
        assert abs(jt.log_evidence - np.log(pe)) <= 1e-12 * abs(np.log(pe))
        both = jt.run_batch([{3: 0}, None])
        assert all(np.array_equal(x, y) for x, y in zip(both[0][0], marg)) and both[0][1] == jt.last["log_evidence"][0]
        assert abs(both[1][1]) <= 1e-12
    finally:
        jt.engine.close()
