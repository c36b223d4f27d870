"""Max-product belief propagation on the GPU (bn_mpe_*, bayesiannetwork_amd/csrc/bn_maxprod.hip) against the host restatement
tests/maxprod_refs.py -- bit for bit: max-marginals, states, sweep counts, residual histories, final messages -- and against the
enumeration of the joint on polytrees.  Both forms (one workgroup, state in LDS; several workgroups, one launch per sweep), batches,
and max-product and sum-product taking turns on one engine.  Every run is bounded by an explicit max_sweeps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxprod_refs  # noqa: E402
from bayesiannetwork_amd import Evidence, synth  # noqa: E402
from bayesiannetwork_amd.dsc import load_dsc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = [2, 3, 4, 3, 2, 4, 5]
SETTINGS = [(1e-3, 50), (1e-9, 50), (1e-9, 1), (1e-9, 2), (1e-9, 5)]   # eps 1e-3 / 1e-9 at 50 sweeps, caps of 1, 2 and 5


def alarm():
    return load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]


# the shapes that reach each ROUNDS instantiation and both wave counts of the one-workgroup kernel
SMALL = {
    "pearl": synth.pearl,
    "resume_chain": synth.resume_chain,
    "alarm_shaped": alarm,
    "mixed12": lambda: synth.random_dag(12, 3, 16, MIXED, seed=2),
    "mixed37_4parents": lambda: synth.random_dag(37, 4, 16, MIXED, seed=5),   # 360-entry tables
    "k7": lambda: synth.random_dag(16, 2, 8, [7, 5, 6, 2], seed=8),           # arity above 4
    "grid8": lambda: synth.grid(8, 8, 4, seed=1),                             # four rounds
    "mixed60": lambda: synth.random_dag(60, 3, 16, MIXED, seed=9),            # 16 waves
}
MID = {
    "mixed80": lambda: synth.random_dag(80, 3, 16, MIXED, seed=10),
    "mixed300": lambda: synth.random_dag(300, 3, 16, MIXED, seed=12),
    "dag60k4_4parents": lambda: synth.random_dag(60, 4, 16, 4, seed=5),       # 1 024-entry tables
    "k7_120": lambda: synth.random_dag(120, 2, 8, [7, 5, 6, 2], seed=8),
}


def hard(model, frac, seed):
    ev = synth.random_evidence(model, frac, seed=seed)
    return ev if ev.ne else Evidence.from_dict(model, {model.n - 1: 0})


def soft(model, seed=3):
    v = model.n // 2
    w = 0.1 + synth.uniform01(seed, 0, int(model.k[v]))
    if model.k[v] > 2:
        w[1] = 0.0
    return Evidence.from_dict(model, {v: w})


def zero_vector(model):
    """an all-zero evidence vector: 0 / 0 in that node's belief and in whatever its messages reach -- NaNs that must match"""
    v = model.n // 3
    return Evidence.from_dict(model, {v: np.zeros(int(model.k[v])), model.n - 1: 0} if v != model.n - 1 else {v: np.zeros(int(model.k[v]))})


def evidences(model):
    return {"none": None, "hard10": hard(model, 0.1, 7), "hard30": hard(model, 0.3, 11), "soft": soft(model), "zero": zero_vector(model)}


def same_bits(got, want, eng=None, what=""):
    assert got["sweeps"] == want["sweeps"], (what, got["sweeps"], want["sweeps"])
    assert got["converged"] == want["converged"], what
    assert np.array_equal(got["max_marginals"], want["beliefs"], equal_nan=True), what
    assert np.array_equal(got["states"], want["states"]), what
    assert got["residual"] == want["residuals"][-1], what
    if eng is not None:
        assert np.array_equal(eng.mpe_residuals(0), want["residuals"]), what
        pi, lam = eng.mpe_messages()
        assert np.array_equal(pi, want["pi_msg"], equal_nan=True) and np.array_equal(lam, want["lambda_msg"], equal_nan=True), what


def check_form(model, form, ev_names=("none", "hard10", "hard30", "soft", "zero"), evs=None):
    """evs: {name: evidence} to take `ev_names` from instead of evidences(model)"""
    from bayesiannetwork_amd.engine import Engine
    evs = evidences(model) if evs is None else evs
    with Engine(model, device=0) as eng:
        eng.set_option("mpe_form", form)
        assert eng.info("mpe_form") == form
        for name in ev_names:
            wants = maxprod_refs.run_settings(model, evs[name], SETTINGS, mode="max")   # one trajectory, shared by the settings
            for (eps, cap), want in zip(SETTINGS, wants):
                for rep in range(3):   # (nothing leaks from run to run)
                    got = eng.mpe_run(evs[name], eps, cap)
                    same_bits(got, want, eng, f"{model.name} {name} eps={eps} cap={cap} run {rep}")
                    assert eng.info("mpe_last_form") == form
        return eng.info("mpe_parts")


@pytest.mark.parametrize("name", list(SMALL))
def test_one_workgroup_form_equals_the_restatement(name):
    check_form(SMALL[name](), 1)


@pytest.mark.parametrize("name", list(MID))
def test_several_workgroup_form_equals_the_restatement(name):
    parts = check_form(MID[name](), 2, ev_names=("none", "hard10", "soft", "zero"))
    if name in ("mixed300", "k7_120", "mixed80"):
        assert parts >= 2   # cross-workgroup state and the device-side stop are exercised


def test_stop_in_the_middle_of_a_launch_group():
    """several-workgroup form: the launches queued behind the stopping sweep are no-ops -- exact sweep counts and states when the run
    converges, or is cut by the cap, in the middle of a group"""
    from bayesiannetwork_amd.engine import Engine
    model = MID["k7_120"]()
    ev = hard(model, 0.3, 11)   # (max-product oscillates on most loopy cases here; this one converges, after 46 sweeps)
    want = maxprod_refs.run(model, ev, 1e-3, 50)
    assert want["converged"] and want["sweeps"] > 8
    with Engine(model, device=0) as eng:
        eng.set_option("mpe_form", 2)
        for group in (3, 4, 5, 7, 8):
            eng.set_option("mpe_group", group)
            got = eng.mpe_run(ev, 1e-3, 50)
            same_bits(got, want, eng, f"group {group}")
            assert eng.info("mpe_last_groups") == -(-want["sweeps"] // group)
        assert any(want["sweeps"] % g != 0 for g in (3, 4, 5, 7, 8))           # ... really in the middle of one
        eng.set_option("mpe_group", 4)
        for cap in (1, 3, 5, 6):                                               # the cap: never converged at eps = 0, cut inside a group
            cut = maxprod_refs.run(model, ev, 0.0, cap)
            got = eng.mpe_run(ev, 0.0, cap)
            assert not got["converged"] and got["sweeps"] == cap
            same_bits(got, cut, eng, f"cap {cap}")


@pytest.mark.parametrize("name", ["alarm_shaped", "mixed37_4parents", "grid8"])
def test_both_forms_agree_bit_for_bit(name):
    from bayesiannetwork_amd.engine import Engine
    model = SMALL[name]()
    with Engine(model, device=0) as eng:
        eng.set_option("mpe_form", 2)   # (a network one workgroup holds: max-product builds a several-workgroup plan of its own)
        assert eng.info("mpe_form") == 2 and eng.info("mpe_parts") >= 2, f"{name} has no several-workgroup plan"
        for ev in (None, hard(model, 0.1, 7), soft(model)):
            eng.set_option("mpe_form", 1)
            a = eng.mpe_run(ev, 1e-9, 30)
            ra, ma = eng.mpe_residuals(0), eng.mpe_messages()
            eng.set_option("mpe_form", 2)
            b = eng.mpe_run(ev, 1e-9, 30)
            assert eng.info("mpe_last_form") == 2
            assert a["sweeps"] == b["sweeps"] and np.array_equal(a["states"], b["states"])
            assert np.array_equal(a["max_marginals"], b["max_marginals"], equal_nan=True)
            assert np.array_equal(ra, eng.mpe_residuals(0))
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ma, eng.mpe_messages()))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("n,seed,n_ev", maxprod_refs.POLYTREE_CASES)
def test_exact_on_polytrees(n, seed, n_ev, form):
    """the cases of tests/test_maxprod_refs.py through the device: max-marginals within 1e-12 of the enumeration, the decoded states its
    argmax (every case has a relative margin of 1e-9 between the best and the second-best joint), log-probability = log of the best"""
    import exact_refs
    from bayesiannetwork_amd.engine import MaxProduct
    model, ev, ev_state = maxprod_refs.polytree_case(n, seed, n_ev)
    want, want_states, best, second = maxprod_refs.brute_max_marginals(model, ev_state)
    assert best > 0.0 and second < best * (1.0 - 1e-9)
    mp = MaxProduct(model, device=0)
    try:
        mp.engine.set_option("mpe_form", form)
        assert mp.engine.info("mpe_form") == form, "the polytree is not eligible for this form"
        cap = exact_refs.skeleton_diameter(model) + 2
        mm = mp(ev, 1e-12, cap)
        assert mp.engine.info("mpe_last_form") == form
        err = float(np.abs(np.concatenate(mm) - want).max())
        print(f"polytree n={n} seed={seed} evidence={n_ev} form {form}: max |max-marginal - enumeration| = {err:.3e}")
        assert err <= 1e-12
        states, logp = mp.mpe(ev, 1e-12, cap)
        assert np.array_equal(states, want_states)
        assert abs(logp - np.log(best)) <= 1e-12 * abs(np.log(best))
    finally:
        mp.engine.close()


def mixed_sets(model, count):
    """evidence sets of a batch: an empty one, hard, soft and one that produces NaNs, then hard sets of other seeds"""
    base = [None, hard(model, 0.1, 7), soft(model), zero_vector(model), hard(model, 0.3, 11)]
    return (base + [hard(model, 0.1 + 0.02 * (q % 5), 20 + q) for q in range(max(0, count - len(base)))])[:count]


@pytest.mark.parametrize("form,counts", [(1, (1, 2, 17, 64)), (2, (1, 2, 5))])
def test_batches_have_the_bits_of_single_runs(form, counts):
    from bayesiannetwork_amd.engine import Engine
    model = alarm()
    with Engine(model, device=0) as eng:
        eng.set_option("mpe_form", form)
        sets = mixed_sets(model, max(counts))
        singles = []
        for ev in sets:
            r = eng.mpe_run(ev, 1e-6, 40)
            r["hist"] = eng.mpe_residuals(0)
            singles.append(r)
        assert np.isnan(singles[3]["max_marginals"]).any()   # (the all-zero vector's set)
        for count in counts:
            out = eng.mpe_run_batch(sets[:count], 1e-6, 40)
            assert eng.info("mpe_last_form") == form
            for q in range(count):
                one = singles[q]
                assert out["sweeps"][q] == one["sweeps"] and out["residual"][q] == one["residual"] and out["converged"][q] == one["converged"]
                assert np.array_equal(out["max_marginals"][q], one["max_marginals"], equal_nan=True), (count, q)
                assert np.array_equal(out["states"][q], one["states"]), (count, q)
                assert np.array_equal(eng.mpe_residuals(q), one["hist"]), (count, q)
    # ... and the single runs are the restatement's
    for ev, one in list(zip(sets, singles))[:5]:
        same_bits(one, maxprod_refs.run(model, ev, 1e-6, 40))


@pytest.mark.parametrize("form", [1, 2])
def test_max_product_and_sum_product_take_turns(form, oracle_mod):
    """one engine: bp_run, mpe_run, bp_run_batch, mpe_run_batch -- then reload_cpt and the same again.  Every sum-product result is the
    oracle's bit for bit and takes the path it takes without the max-product calls in between; every max-product result is the
    restatement's; bn_bp_messages still reads the sum-product run."""
    from bayesiannetwork_amd import FlatModel
    from bayesiannetwork_amd.engine import Engine
    model = alarm()
    evs = [hard(model, 0.1, 7), soft(model), None]
    with Engine(model, device=0) as plain:   # the paths without any max-product call
        plain.bp_run(evs[0], 1e-6)
        path_single = plain.last_path()
        plain.bp_run_batch(evs, 1e-6)
        path_batch = plain.last_path()
    with Engine(model, device=0) as eng:
        eng.set_option("mpe_form", form)
        for rnd in range(2):
            cur = eng.model
            for turn in range(2):
                ev = evs[turn]
                want = oracle_mod.bp_run(cur, ev, 1e-6, dump_msgs=True)
                got = eng.bp_run(ev, 1e-6)
                assert got["sweeps"] == want["sweeps"] and np.array_equal(got["beliefs"], want["beliefs"])
                assert eng.last_path() == path_single
                m = eng.mpe_run(evs[1 - turn], 1e-6, 40)
                same_bits(m, maxprod_refs.run(cur, evs[1 - turn], 1e-6, 40), eng)
                assert eng.last_path() == path_single
                pi, lam = eng.bp_messages()            # still the sum-product run's
                assert np.array_equal(pi, want["pi_msg"]) and np.array_equal(lam, want["lambda_msg"])
                assert np.array_equal(eng.bp_residuals(), want["residuals"])
                again = eng.bp_run_device(1e-6)        # the evidence in force is still the sum-product call's
                assert again["sweeps"] == want["sweeps"] and np.array_equal(eng.bp_beliefs(), want["beliefs"])
                out = eng.bp_run_batch(evs, 1e-6)
                assert eng.last_path() == path_batch
                mb = eng.mpe_run_batch(evs, 1e-6, 40)
                assert eng.last_path() == path_batch
                for q, e2 in enumerate(evs):
                    w = oracle_mod.bp_run(cur, e2, 1e-6)
                    assert out["sweeps"][q] == w["sweeps"] and np.array_equal(out["beliefs"][q], w["beliefs"])
                    r = maxprod_refs.run(cur, e2, 1e-6, 40)
                    assert mb["sweeps"][q] == r["sweeps"] and np.array_equal(mb["states"][q], r["states"])
                    assert np.array_equal(mb["max_marginals"][q], r["beliefs"], equal_nan=True)
                assert np.array_equal(eng.bp_beliefs_batch(), out["beliefs"])   # the batch's results are still there
            if rnd == 0:   # new tables on the same structure: both kinds of run must see them
                rng = np.random.default_rng(3)
                cpt = cur.cpt.copy()
                for v in range(cur.n):
                    t = cpt[int(cur.cpt_off[v]):int(cur.cpt_off[v + 1])].reshape(-1, int(cur.k[v]))
                    t *= 0.5 + rng.random(t.shape)
                    t /= t.sum(axis=1, keepdims=True)
                eng.reload_cpt(cpt)
                assert isinstance(eng.model, FlatModel) and not np.array_equal(eng.model.cpt, cur.cpt)
