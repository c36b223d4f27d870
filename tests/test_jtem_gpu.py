"""Exact expectation-maximisation on the GPU (bn_jt_em_* of include/bn_mi355x.h; Engine.jt_em_expected_counts / jt_em_fit,
JunctionTree.em_fit, jt_em_fit) against the numpy restatement tests/jtem_refs.py: E, theta after every iteration, the delta history and
the skipped count BIT FOR BIT; ll_p and L within 1e-12 of sum |count x log scale| (the device's log is not numpy's: the bound of
tests/test_jtree_gpu.py for log P(e)).  Both forms, launch edges inside a block of the E sum, the kinds of rows a table may hold, a
complete table, the ALARM-shaped network, cross-checks against bn_em_expected_counts and bn_jt_run_batch, and the calls around a fit."""
import numpy as np
import pytest

from bayesiannetwork_amd import _lib, from_parent_lists, synth
from bayesiannetwork_amd import engine as eng_mod
from bayesiannetwork_amd.engine import Engine, JunctionTree

import em_refs
import exact_refs as xr
import jtem_refs
import jtree_refs as jr

pytestmark = pytest.mark.gpu

M = em_refs.MISSING


def close_ll(got, want, bound):
    """-inf equals -inf; else within 1e-12 of the sum of the terms' magnitudes."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all((got == want) | (np.abs(got - want) <= 1e-12 * bound)))


def check_estep(e, model, plan, pats, counts, what):
    want = jtem_refs.expected_counts(model, plan, pats, counts)
    E, ll = e.jt_em_expected_counts(pats, counts)
    finite = np.isfinite(want["loglik"])
    print(what, "rows", len(counts), "max |ll - ref|", float(np.abs(ll[finite] - want["loglik"][finite]).max()) if finite.any() else 0.0)
    assert jr.same_bits(E, want["E"]), (what, "E", float(np.nanmax(np.abs(E - want["E"]))))
    assert e.info("jt_em_skipped") == want["skipped"], (what, "skipped")
    assert close_ll(ll, want["loglik"], want["row_bound"]), (what, "ll_p")
    assert e.info("jt_em_last_iters") == 1
    return want


def check_fit(e, model, plan, pats, counts, what, **kw):
    want = jtem_refs.em_fit(model, plan, pats, counts, **kw)
    thetas, deltas, Ls = [], [], []
    init = kw.get("cpt_init")
    for it in range(want["iters"]):   # theta after EVERY iteration: one iteration per call, continued from the last tables
        cpt, iters, hist, lls = e.jt_em_fit(pats, counts, max_iters=1, tol=0.0, prior=kw.get("prior", 0.0), cpt_init=init)
        assert iters == 1
        thetas.append(cpt)
        deltas.append(hist[0])
        Ls.append(lls[0])
        init = cpt
    for it in range(want["iters"]):
        assert jr.same_bits(thetas[it], want["thetas"][it]), (what, "theta after iteration", it)
        assert close_ll(Ls[it], want["L"][it], want["bounds"][it]), (what, "L", it, Ls[it], want["L"][it])
    assert jr.same_bits(deltas, want["deltas"]), (what, "deltas")
    # ... and the whole loop in one call
    cpt, iters, hist, lls = e.jt_em_fit(pats, counts, **kw)
    assert iters == want["iters"] and jr.same_bits(cpt, want["cpt"]) and jr.same_bits(hist, want["deltas"]), what
    assert close_ll(lls, want["L"], want["bounds"]), (what, "L history")
    assert e.info("jt_em_skipped") == want["skipped"] and e.info("jt_em_last_iters") == want["iters"]
    return want


NETS = {"pearl": synth.pearl, "grid3x3k2": lambda: synth.grid(3, 3, 2, seed=1), "dag12": lambda: synth.random_dag(12, 3, 6, [2, 3], seed=4)}


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", sorted(NETS))
def test_both_forms_equal_the_restatement(bnlib, name, form):
    model = NETS[name]()
    pats, counts = em_refs.sampled_table(model, 40, 0.35, seed=310)
    init = em_refs.random_positive_cpt(model, 31)
    with Engine(model, device=0) as e:
        assert e.info("jt_form") == 1
        e.set_option("jt_form", 0 if form == 1 else 2)
        plan = e.jt_plan()
        check_estep(e, model, plan, pats, counts, (name, form))
        assert e.info("jt_em_last_form") == form and e.info("jt_em_last_launches") == 1
        check_fit(e, model, plan, pats, counts, (name, form), max_iters=3, tol=0.0, cpt_init=init)
        assert e.info("jt_em_estep_ns") > 0 and e.info("jt_em_mstep_ns") > 0


def test_a_plan_that_is_form_2_by_itself(bnlib):
    model = xr.wide(12)
    pats, counts = em_refs.sampled_table(model, 5, 0.4, seed=311)
    pats = np.concatenate([pats, np.full((1, model.n), M, np.uint8)])
    counts = np.concatenate([counts, np.asarray([2], np.uint64)])
    with Engine(model, device=0) as e:
        assert e.info("jt_form") == 2
        plan = e.jt_plan()
        check_estep(e, model, plan, pats, counts, "wide12")
        assert e.info("jt_em_last_form") == 2
        e.set_option("jt_scratch_cells", 2 * plan["state_cells"] + 5)   # two rows per launch
        check_estep(e, model, plan, pats, counts, "wide12, two rows per launch")
        assert e.info("jt_em_last_launches") == (len(counts) + 1) // 2
        check_fit(e, model, plan, pats, counts, "wide12", max_iters=2, tol=0.0, prior=0.5)


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 513])
def test_row_counts_and_launch_edges_inside_a_block(bnlib, rows):
    model = synth.pearl()
    rng = np.random.default_rng(rows)
    pats = rng.integers(0, 2, size=(rows, model.n)).astype(np.uint8)
    pats[rng.random(pats.shape) < 0.4] = M
    counts = rng.integers(0, 9, size=rows).astype(np.uint64)
    counts[0] = 3
    S = int(model.cpt_off[-1])
    with Engine(model, device=0) as e:
        plan = e.jt_plan()
        want = check_estep(e, model, plan, pats, counts, ("pearl", rows))
        e.set_option("jt_em_scratch_cells", 100 * S + 3)   # 100 rows per launch: edges at 100, 200, 300, ... inside the blocks of 256
        E, ll = e.jt_em_expected_counts(pats, counts)
        assert e.info("jt_em_last_launches") == (rows + 99) // 100
        assert jr.same_bits(E, want["E"]) and close_ll(ll, want["loglik"], want["row_bound"])
        check_fit(e, model, plan, pats, counts, ("pearl, cut", rows), max_iters=2, tol=0.0, prior=0.25)


def test_row_kinds_in_one_table(bnlib):
    model = xr.disjoint_union([synth.pearl(), synth.pearl()], name="two_pearls")
    # pearl: W (node 2) is 0 whenever R (node 0) is 0, so R = 0, W = 1 has probability 0 -- in the first tree only
    assert float(synth.pearl().cpt_of(2).ravel()[1]) == 0.0
    pats = np.asarray([[1, 1, 1, 1, 1, M, 1, 1],      # a 2^40 count
                       [1, M, 0, 1, M, M, 1, 0],      # count 0
                       [M] * 8,                       # fully missing
                       [0, M, 1, M, 1, 0, M, 0],      # probability 0 in the first tree
                       [1, 0, M, 0, 1, 0, 1, M]], np.uint8)
    counts = np.asarray([1 << 40, 0, 5, 2, 7], np.uint64)
    with Engine(model, device=0) as e:
        plan = e.jt_plan()
        assert int((plan["parent"] < 0).sum()) == 2
        b, skipped, _ = jtem_refs.ExactE(model, plan).row(pats[3])
        half = int(model.cpt_off[4])
        assert skipped == 4 and not b[:half].any() and b[half:].any()   # only the first tree's four families
        want = check_estep(e, model, plan, pats, counts, "row kinds")
        assert want["skipped"] == 4 and want["L"] == -np.inf and want["loglik"][3] == -np.inf and abs(want["loglik"][2]) <= 1e-12
        init = em_refs.random_positive_cpt(model, 33)
        cpt, iters, hist, lls = e.jt_em_fit(pats, counts, max_iters=1, tol=0.0)
        assert lls[0] == -np.inf and e.info("jt_em_skipped") == 4
        check_fit(e, model, plan, pats, counts, "row kinds, the tables with zeros", max_iters=2, tol=0.0)
        check_fit(e, model, plan, pats, counts, "row kinds, positive tables", max_iters=2, tol=0.0, cpt_init=init)


def test_complete_table_gives_the_counts_and_the_cpt_fit(bnlib):
    model = synth.grid(3, 3, 2, seed=1)
    pats, counts = em_refs.sampled_table(model, 300, 0.0, seed=51)
    counts = counts * np.uint64(3) + np.uint64(1)
    with Engine(model, device=0) as e:
        E, _ = e.jt_em_expected_counts(pats, counts)
        fitted = eng_mod.fit_cpt(model, pats, counts, device=0)
        cpt, iters, _, _ = e.jt_em_fit(pats, counts, max_iters=1, tol=0.0)
    want = np.zeros(int(model.cpt_off[-1]), np.uint64)
    for v in range(model.n):
        row = np.zeros(len(counts), np.int64)
        for u in model.parents(v):
            row = row * int(model.k[u]) + pats[:, int(u)]
        np.add.at(want, int(model.cpt_off[v]) + row * int(model.k[v]) + pats[:, v], counts)
    assert np.array_equal(E, want.astype(np.float64))
    assert iters == 1 and jr.same_bits(cpt, fitted)


def test_alarm_shaped_two_iterations(bnlib):
    model = jr.alarm()
    pats, counts = em_refs.sampled_table(model, 64, 0.25, seed=305)
    assert len(counts) == 64
    init = em_refs.random_positive_cpt(model, 25)
    with Engine(model, device=0) as e:
        plan = e.jt_plan()
        check_fit(e, model, plan, pats, counts, "alarm", max_iters=2, tol=0.0, cpt_init=init)
    cpt, iters, _, _ = eng_mod.jt_em_fit(model, pats, counts, device=0, max_iters=2, tol=0.0, cpt_init=init)
    with Engine(model, device=0) as e:
        again = e.jt_em_fit(pats, counts, max_iters=2, tol=0.0, cpt_init=init)[0]
    assert iters == 2 and jr.same_bits(cpt, again)


def test_polytree_matches_the_belief_propagation_estep(bnlib):
    model = synth.pearl()
    pats, counts = em_refs.sampled_table(model, 12, 0.4, seed=77)
    counts = np.minimum(counts, np.uint64(3))
    with Engine(model, device=0) as e:
        E, _ = e.jt_em_expected_counts(pats, counts)
        bp, _ = e.em_expected_counts(pats, counts, bp_eps=1e-12)
    print("pearl: max |E exact - E belief propagation| =", float(np.abs(E - bp).max()))
    assert np.abs(E - bp).max() <= 1e-12


def test_grid_matches_the_junction_tree_marginals(bnlib):
    model = synth.grid(3, 3, 4, seed=1)
    pats, _ = em_refs.sampled_table(model, 5, 0.4, seed=78)
    one = np.asarray([1], np.uint64)
    with Engine(model, device=0) as e:
        ref = e.jt_run_batch([em_refs.evidence_of(model, row) for row in pats])
        for p, row in enumerate(pats):
            b, ll = e.jt_em_expected_counts(row[None, :], one)   # one row of count 1: E is the row's posteriors
            for v in range(model.n):
                own = b[int(model.cpt_off[v]):int(model.cpt_off[v + 1])].reshape(-1, int(model.k[v])).sum(axis=0)
                assert np.abs(own - ref["beliefs"][p][model.node_off[v]:model.node_off[v + 1]]).max() <= 1e-12
            with np.errstate(divide="ignore"):
                bound = float(np.abs(np.log(ref["scales"][p])).sum())
            assert abs(ll[0] - ref["log_evidence"][p]) <= 1e-12 * bound


def test_a_fit_leaves_the_other_call_families_alone(bnlib):
    model = from_parent_lists([2, 2, 2, 2], [[], [], [0], [0, 1]],
                              [[0.3, 0.7], [0.4, 0.6], [0.9, 0.1, 0.2, 0.8], [0.7, 0.3, 0.6, 0.4, 0.8, 0.2, 0.1, 0.9]], name="pearl_positive")
    pats, counts = em_refs.sampled_table(model, 30, 0.3, seed=79)
    ev = em_refs.evidence_of(model, np.asarray([M, 1, M, 0], np.uint8))
    with Engine(model, device=0) as a:
        alone_jt = a.jt_run(ev)
    with Engine(model, device=0) as a:
        alone_mpe = a.jt_mpe_run(ev)
    with Engine(model, device=0) as a:
        alone_bp = a.bp_run(ev, 1e-9)
    with Engine(model, device=0) as a:
        alone_em = a.em_fit(pats, counts, max_iters=3, tol=0.0)
    with Engine(model, device=0) as a:
        alone_fit = a.jt_em_fit(pats, counts, max_iters=3, tol=0.0)
    with Engine(model, device=0) as e:
        def fit_between():
            kind, scales = e.info("jt_last_kind"), (e.jt_scales(0) if e.info("jt_last_kind") else None)
            forms = (e.info("jt_last_form"), e.info("jt_last_launches"))
            got = e.jt_em_fit(pats, counts, max_iters=3, tol=0.0)
            assert all(jr.same_bits(x, y) for x, y in zip(got[2:3], alone_fit[2:3])) and jr.same_bits(got[0], alone_fit[0])
            assert e.info("jt_last_kind") == kind and forms == (e.info("jt_last_form"), e.info("jt_last_launches"))
            if kind:
                assert jr.same_bits(e.jt_scales(0), scales)
            else:
                with pytest.raises(_lib.BnError):
                    e.jt_scales(0)
        fit_between()
        got = e.jt_run(ev)
        assert jr.same_bits(got["beliefs"], alone_jt["beliefs"]) and jr.same_bits(got["scales"], alone_jt["scales"])
        fit_between()
        assert e.info("jt_last_kind") == 1
        got = e.jt_mpe_run(ev)
        assert np.array_equal(got["states"], alone_mpe["states"]) and jr.same_bits(got["max_marginals"], alone_mpe["max_marginals"])
        assert jr.same_bits(got["scales"], alone_mpe["scales"])
        fit_between()
        assert e.info("jt_last_kind") == 2
        got = e.bp_run(ev, 1e-9)
        assert jr.same_bits(got["beliefs"], alone_bp["beliefs"]) and got["sweeps"] == alone_bp["sweeps"]
        fit_between()
        got = e.em_fit(pats, counts, max_iters=3, tol=0.0)
        assert jr.same_bits(got[0], alone_em[0]) and jr.same_bits(got[2], alone_em[2])
        fit_between()
        got = e.jt_run(ev)   # the engine's own potentials are those of its own tables still
        assert jr.same_bits(got["beliefs"], alone_jt["beliefs"])


EM_INFO = ("em_eligible", "em_last_iters", "em_capped", "em_skipped", "em_estep_ns", "em_mstep_ns", "em_scratch_cells")
JT_EM_INFO = ("jt_em_last_iters", "jt_em_skipped", "jt_em_estep_ns", "jt_em_mstep_ns", "jt_em_last_form", "jt_em_last_launches",
              "jt_em_scratch_cells")


def test_the_two_fits_share_the_loop_and_no_state(bnlib):
    """em_fit, jt_em_fit, em_fit on one engine: the two families run the same loop over states of their own.  257 rows (a block edge
    inside the table), 100 rows per launch on both paths (launch edges inside a block)."""
    from test_em_gpu import random_table, tiny
    model = tiny("collider")
    pats, counts = random_table(model, 257, 0.3, seed=257)
    S = int(model.cpt_off[-1])
    want_bp = em_refs.em_fit(model, pats, counts, max_iters=2, tol=0.0)
    with Engine(model, device=0) as e:
        want_jt = jtem_refs.em_fit(model, e.jt_plan(), pats, counts, max_iters=2, tol=0.0)
        e.set_option("em_scratch_cells", 100 * S)
        e.set_option("jt_em_scratch_cells", 100 * S + 3)
        info = lambda names: {name: e.info(name) for name in names}

        def bp_fit():
            cpt, iters, hist = e.em_fit(pats, counts, max_iters=2, tol=0.0)
            assert iters == want_bp["iters"] and np.array_equal(cpt, want_bp["cpt"], equal_nan=True) and np.array_equal(hist, want_bp["deltas"])
            assert e.info("em_capped") == want_bp["capped"] and e.info("em_skipped") == want_bp["skipped"]
            return cpt, hist, [e.info(name) for name in ("em_last_iters", "em_capped", "em_skipped")]

        first = bp_fit()
        em_before, jt_start = info(EM_INFO), info(JT_EM_INFO)
        cpt, iters, hist, lls = e.jt_em_fit(pats, counts, max_iters=2, tol=0.0)
        assert iters == want_jt["iters"] and jr.same_bits(cpt, want_jt["cpt"]) and jr.same_bits(hist, want_jt["deltas"])
        assert close_ll(lls, want_jt["L"], want_jt["bounds"])
        assert e.info("jt_em_skipped") == want_jt["skipped"] and e.info("jt_em_last_iters") == want_jt["iters"]
        assert e.info("jt_em_last_launches") == 3
        assert info(EM_INFO) == em_before                      # the tree's fit wrote nothing the em_* names read
        jt_before = info(JT_EM_INFO)
        assert jt_before != jt_start
        third = bp_fit()
        assert info(JT_EM_INFO) == jt_before                   # ... and the other way round
        assert jr.same_bits(first[0], third[0]) and jr.same_bits(first[1], third[1]) and first[2] == third[2]


def test_junction_tree_functor_and_reload(bnlib):
    model = synth.grid(3, 3, 2, seed=1)
    pats, counts = em_refs.sampled_table(model, 40, 0.3, seed=80)
    with Engine(model, device=0) as e:
        want = e.jt_em_fit(pats, counts, max_iters=3, tol=0.0)
    jt = JunctionTree(model, device=0)
    got = jt.em_fit(pats, counts, max_iters=3, tol=0.0, reload=True)
    assert jr.same_bits(got[0], want[0]) and got[1] == 3 and len(got[3]) == 3
    assert jr.same_bits(jt.engine.model.cpt, want[0]) and jr.same_bits(jt.model.cpt, want[0])
    with Engine(em_refs.with_cpt(model, want[0]), device=0) as e:
        fresh = e.jt_run(None)
    assert jr.same_bits(jt.engine.jt_run(None)["beliefs"], fresh["beliefs"])   # the reload reached the junction tree's potentials
    jt.engine.close()
