"""Expectation-maximisation on the GPU (bn_em_*, bayesiannetwork_amd/csrc/bn_em.hip) against the host restatement tests/em_refs.py --
bit for bit: the expected counts E, the tables after every iteration, the delta history, the per-pattern sweep counts, the iteration
count, the counters of capped runs and skipped families.  The restatement is slow, so the sizes are the smallest that reach each
branch: both sides of the 256-block of the E sum with launch edges forced inside a block, every row kind in one table, the kernel's
one-, two- and four-round instantiations, the eight-parent edge, a capped loopy run; and an EM call between sum-product and
max-product calls on one engine changes nothing of theirs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import em_refs  # noqa: E402
import maxprod_refs  # noqa: E402
from bayesiannetwork_amd import Evidence, from_parent_lists, synth  # noqa: E402
from bayesiannetwork_amd.dsc import load_dsc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = [2, 3, 4, 3, 2, 4, 5]
M = em_refs.MISSING


def alarm():
    return load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]


def _tables(k, parents, seed):
    rng = np.random.default_rng(seed)
    cpts = []
    for v, ps in enumerate(parents):
        rows = int(np.prod([k[u] for u in ps])) if ps else 1
        t = 0.1 + rng.random((rows, k[v]))
        cpts.append((t / t.sum(axis=1, keepdims=True)).ravel())
    return cpts


def tiny(name):
    k, parents = {"root": ([3], [[]]), "chain2": ([2, 3], [[], [0]]), "collider": ([2, 3, 4], [[], [], [0, 1]])}[name]
    return from_parent_lists(k, parents, _tables(k, parents, seed=7), name=name)


def eight_parents():
    k, parents = [2] * 9, [[] for _ in range(8)] + [list(range(8))]
    return from_parent_lists(k, parents, _tables(k, parents, seed=8), name="eight_parents")


def random_table(model, rows, blank, seed, max_count=5):
    """`rows` rows in a fixed order: forward-sample-free random states, a fraction `blank` of the cells not observed, counts 0..max_count
    (the last one at least 1: the total is never zero)."""
    rng = np.random.default_rng(seed)
    pats = np.stack([rng.integers(0, int(kk), rows) for kk in model.k], axis=1).astype(np.uint8)
    pats[rng.random(pats.shape) < blank] = M
    counts = rng.integers(0, max_count + 1, rows).astype(np.uint64)
    counts[-1] = max(int(counts[-1]), 1)
    return np.ascontiguousarray(pats), counts


def check_against_restatement(model, pats, counts, scratch_rows=None, what="", **kw):
    """One E-step under the model's tables, then em_fit cut after 1, 2, ... iterations, against em_refs.em_fit: every figure bit for bit.
    scratch_rows: the scratch array is limited to that many rows per launch."""
    from bayesiannetwork_amd.engine import Engine
    kw = dict({"max_iters": 2, "tol": 0.0, "bp_eps": 1e-3, "bp_max_sweeps": 0, "prior": 0.0}, **kw)
    want = em_refs.em_fit(model, pats, counts, **kw)
    S = int(model.cpt_off[-1])
    with Engine(model, device=0) as eng:
        assert eng.info("em_eligible") == 1
        if scratch_rows is not None:
            eng.set_option("em_scratch_cells", scratch_rows * S)
        if kw.get("cpt_init") is None:
            E, sweeps = eng.em_expected_counts(pats, counts, kw["bp_eps"], kw["bp_max_sweeps"])
            assert np.array_equal(sweeps, want["sweeps"][0]), what
            assert np.array_equal(E, want["E"][0], equal_nan=True), what
            assert eng.info("em_last_iters") == 1
        for stop in range(1, want["iters"] + 1):
            cpt, iters, hist = eng.em_fit(pats, counts, **dict(kw, max_iters=stop))
            assert iters == stop and eng.info("em_last_iters") == stop, what
            assert np.array_equal(cpt, want["thetas"][stop - 1], equal_nan=True), (what, stop)
            assert np.array_equal(hist, want["deltas"][:stop]), (what, stop)
        # the whole call, with the caller's stopping rule
        cpt, iters, hist = eng.em_fit(pats, counts, **kw)
        assert iters == want["iters"] and np.array_equal(cpt, want["cpt"], equal_nan=True) and np.array_equal(hist, want["deltas"]), what
        assert eng.info("em_capped") == want["capped"] and eng.info("em_skipped") == want["skipped"], what
        assert eng.info("em_estep_ns") > 0 and eng.info("em_mstep_ns") > 0
        assert np.array_equal(eng.model.cpt, model.cpt)   # the engine's own tables were never written
        # the last iteration's E-step once more, through the tables before it: expected counts and sweep counts of a LATER iteration
        if want["iters"] >= 2 and kw.get("cpt_init") is None:
            eng.reload_cpt(want["thetas"][want["iters"] - 2])
            E, sweeps = eng.em_expected_counts(pats, counts, kw["bp_eps"], kw["bp_max_sweeps"])
            assert np.array_equal(sweeps, want["sweeps"][-1]) and np.array_equal(E, want["E"][-1], equal_nan=True), what
    return want


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("name", ["root", "chain2", "collider"])
def test_tiny_networks_on_both_sides_of_the_block(name, rows):
    model = tiny(name)
    pats, counts = random_table(model, rows, 0.3, seed=rows)
    # 100 rows per launch: launch edges at 100, 200, ... fall inside the 256-blocks; then the whole table in one launch
    a = check_against_restatement(model, pats, counts, scratch_rows=100, what=f"{name} {rows} rows, 100 per launch")
    b = check_against_restatement(model, pats, counts, what=f"{name} {rows} rows, one launch")
    assert np.array_equal(a["cpt"], b["cpt"])


def test_scratch_limit_below_one_row_still_runs_one_row_per_launch():
    model = tiny("collider")
    pats, counts = random_table(model, 7, 0.3, seed=5)
    from bayesiannetwork_amd.engine import Engine
    want = em_refs.expected_counts(model, pats, counts, 1e-3, 0)
    with Engine(model, device=0) as eng:
        eng.set_option("em_scratch_cells", 1)
        E, sweeps = eng.em_expected_counts(pats, counts)
        assert np.array_equal(E, want["E"]) and np.array_equal(sweeps, want["sweeps"])


def test_every_row_kind_in_one_table():
    """fully observed, fully missing, count 0, a count of 2^40, and a row whose evidence has probability 0 under tables with zeros: that
    row's family is skipped and counted, E holds no NaN, and a CPT row nothing supports falls back to uniform"""
    model = tiny("collider")   # arities 2, 3, 4; node 2 has parents 0 and 1
    init = model.cpt.copy()
    init[0:2] = [1.0, 0.0]                      # P(x0 = 1) = 0
    init[2:5] = [0.25, 0.75, 0.0]               # P(x1 = 2) = 0, and no row observes x1 = 2
    pats = np.asarray([[0, 1, 3], [M, M, M], [0, 0, 1], [M, 1, 2], [1, 0, M], [0, M, M], [M, M, 0]], np.uint8)
    counts = np.asarray([3, 2, 0, 1 << 40, 5, 1, 7], np.uint64)
    want = check_against_restatement(model, pats, counts, what="row kinds", cpt_init=init, max_iters=3)
    assert want["skipped"] > 0 and not np.isnan(np.concatenate(want["E"])).any()
    off2 = int(model.cpt_off[2])
    rows2 = want["thetas"][0][off2:].reshape(6, 4)
    assert np.array_equal(rows2[2], np.full(4, 0.25)) and np.array_equal(rows2[5], np.full(4, 0.25))   # parent assignments (0, 2) and (1, 2)
    assert want["E"][0].max() >= float(1 << 40)
    # ... and from the model's own strictly positive tables nothing is skipped
    again = check_against_restatement(model, pats, counts, what="row kinds, positive tables", prior=0.5)
    assert again["skipped"] == 0


LARGER = {
    "alarm_shaped": (alarm, 1),                                                          # one round of items
    "eight_parents": (eight_parents, 1),                                                 # the kSmallMaxParents edge
    "mixed37_4parents": (lambda: synth.random_dag(37, 4, 16, MIXED, seed=5), 2),         # two rounds of entry items
    "grid8": (lambda: synth.grid(8, 8, 4, seed=1), 3),                                   # the four-round instantiation
}


@pytest.mark.parametrize("name", list(LARGER))
def test_larger_networks(name):
    from bayesiannetwork_amd.engine import Engine
    make, min_rounds = LARGER[name]
    model = make()
    with Engine(model, device=0) as eng:
        plan = eng.small_plan()
        assert plan is not None and plan["re"] >= min_rounds, (name, plan and plan["re"])
        if name == "eight_parents":
            assert plan["mmax"] == 8
    pats, counts = random_table(model, 12 if name == "grid8" else 24, 0.25, seed=31)
    check_against_restatement(model, pats, counts, scratch_rows=10, what=name, bp_max_sweeps=12)


def test_capped_runs_on_a_loopy_grid():
    model = synth.grid(3, 3, 3, seed=4)
    pats, counts = random_table(model, 40, 0.4, seed=9)
    want = check_against_restatement(model, pats, counts, scratch_rows=16, what="grid 3x3, cap 3", bp_eps=1e-9, bp_max_sweeps=3)
    assert want["capped"] > 0 and all((s <= 3).all() for s in want["sweeps"]) and any((s == 3).any() for s in want["sweeps"])


def test_em_between_sum_product_and_max_product_calls(oracle_mod):
    """bp_run with evidence, em_fit, bp_run_device, bp_messages, mpe_run: the EM call changes nothing the others read -- the evidence in
    force, the state bn_bp_messages reads, the path, a staged batch, the engine's tables.  With reload=True the next bp_run is that of an
    engine created on the fitted tables."""
    from bayesiannetwork_amd.engine import Engine
    model = alarm()
    ev = synth.random_evidence(model, 0.1, seed=7)
    ev2 = synth.random_evidence(model, 0.3, seed=11)
    pats, counts = random_table(model, 20, 0.25, seed=3)
    want = oracle_mod.bp_run(model, ev, 1e-6, dump_msgs=True)
    want_mpe = maxprod_refs.run(model, ev2, 1e-6, 40)
    with Engine(model, device=0) as plain:
        plain.bp_run(ev, 1e-6)
        path = plain.last_path()
    with Engine(model, device=0) as eng:
        got = eng.bp_run(ev, 1e-6)
        assert got["sweeps"] == want["sweeps"] and np.array_equal(got["beliefs"], want["beliefs"]) and eng.last_path() == path
        m0 = eng.mpe_run(ev2, 1e-6, 40)
        cpt, iters, _ = eng.em_fit(pats, counts, max_iters=2, tol=0.0, bp_max_sweeps=12)
        assert iters == 2 and not np.array_equal(cpt, model.cpt)
        assert eng.last_path() == path
        pi, lam = eng.bp_messages()                 # still the sum-product run's
        assert np.array_equal(pi, want["pi_msg"]) and np.array_equal(lam, want["lambda_msg"])
        assert np.array_equal(eng.bp_residuals(), want["residuals"])
        again = eng.bp_run_device(1e-6)             # the evidence in force is still the sum-product call's; the tables are the old ones
        assert again["sweeps"] == want["sweeps"] and np.array_equal(eng.bp_beliefs(), want["beliefs"])
        pi, lam = eng.bp_messages()
        assert np.array_equal(pi, want["pi_msg"]) and np.array_equal(lam, want["lambda_msg"])
        m1 = eng.mpe_run(ev2, 1e-6, 40)
        for m in (m0, m1):
            assert m["sweeps"] == want_mpe["sweeps"] and np.array_equal(m["states"], want_mpe["states"])
            assert np.array_equal(m["max_marginals"], want_mpe["beliefs"], equal_nan=True)
        assert np.array_equal(eng.mpe_residuals(0), want_mpe["residuals"])
        batch = eng.bp_run_batch([ev, None, ev2], 1e-6)   # a staged batch and its results outlive an EM call too
        path_batch = eng.last_path()
        eng.em_fit(pats, counts, max_iters=1, tol=0.0, bp_max_sweeps=12)
        assert eng.last_path() == path_batch and np.array_equal(eng.bp_beliefs_batch(), batch["beliefs"])
        eng.bp_run_batch_device(1e-6)                     # (the batch's evidence is still staged)
        assert eng.last_path() == path_batch and np.array_equal(eng.bp_beliefs_batch(), batch["beliefs"])
        assert np.array_equal(eng.model.cpt, model.cpt)
        # the same call with reload=True: the fitted tables are now the engine's
        cpt2, _, _ = eng.em_fit(pats, counts, max_iters=2, tol=0.0, bp_max_sweeps=12, reload=True)
        assert np.array_equal(cpt2, cpt) and np.array_equal(eng.model.cpt, cpt)
        after = eng.bp_run(ev, 1e-6)
    with Engine(em_refs.with_cpt(model, cpt), device=0) as fresh:
        ref = fresh.bp_run(ev, 1e-6)
    assert after["sweeps"] == ref["sweeps"] and np.array_equal(after["beliefs"], ref["beliefs"])
    w2 = oracle_mod.bp_run(em_refs.with_cpt(model, cpt), ev, 1e-6)
    assert after["sweeps"] == w2["sweeps"] and np.array_equal(after["beliefs"], w2["beliefs"])


def test_engines_that_are_not_eligible():
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.engine import Engine
    k, parents = [2] * 10, [[] for _ in range(9)] + [list(range(9))]
    nine = from_parent_lists(k, parents, _tables(k, parents, seed=5), name="nine_parents")
    with Engine(nine, device=0) as eng:
        assert eng.info("em_eligible") == 0
        with pytest.raises(_lib.BnError, match="more than 8 parents") as ei:
            eng.em_fit(np.zeros((1, 10), np.uint8), [1], max_iters=2)
        assert ei.value.code == _lib.BN_ERR_STATE
    mid = synth.random_dag(300, 3, 16, MIXED, seed=12)      # the several-workgroup path's network: no one-workgroup plan
    with Engine(mid, device=0) as eng:
        assert eng.info("small_eligible") == 0
        with pytest.raises(_lib.BnError, match="one workgroup") as ei:
            eng.em_expected_counts(np.zeros((1, 300), np.uint8), [1])
        assert ei.value.code == _lib.BN_ERR_STATE
    with Engine(synth.grid(12, 12, 4, seed=2), device=0, rank=0, nranks=2) as eng:
        with pytest.raises(_lib.BnError, match="sharded") as ei:
            eng.em_fit(np.zeros((1, 144), np.uint8), [1], max_iters=2)
        assert ei.value.code == _lib.BN_ERR_STATE
