"""The host restatement of Gibbs sampling (tests/gibbs_refs.py) checked on the CPU: its Philox block against the oracle's, its
colouring, the two continuity identities, its statistics against exact posteriors, and a case with stuck updates.  The GPU equals
the restatement bit for bit (tests/test_gibbs_gpu.py), so the statistical check needs no GPU."""
import numpy as np
import pytest

from bayesiannetwork_amd import _lib, synth

import exact_refs as xr
import gibbs_refs as gr
import jtree_refs as jr
import many_parents

CHAINS = 4096      # independent draws: the FINAL state of each chain
SWEEPS = 32
PEARL_STUCK_EVIDENCE = {2: 1, 3: 0}     # W = 1, H = 0: see test_stuck_updates_on_pearl_and_the_posterior_all_the_same


def ev_of(model, d):
    ev = np.full(model.n, -1, dtype=np.int32)
    for v, s in d.items():
        ev[v] = s
    return ev


def networks():
    return {
        "pearl": synth.pearl(),
        "grid3x3": synth.grid(3, 3, k=3),
        "dag12": synth.random_dag(12, max_parents=3, window=6, k=3, seed=5),
        "alarm": jr.alarm(),
        "star70": xr.star(70, 3, 2),
        "fan5_8": many_parents.fan([5, 8], kp=2, kc=7),
    }


def test_philox_block_equals_the_oracle(oracle_mod):
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, size=(300, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, size=(300, 2), dtype=np.uint64)
    ctr[0], key[0] = 0, 0
    ctr[1], key[1] = 0xFFFFFFFF, 0xFFFFFFFF
    for c, k in zip(ctr, key):
        got = [int(x[0]) for x in gr.philox4x32_10([int(x) for x in c], [int(x) for x in k])]
        assert got == oracle_mod.philox([int(x) for x in c], [int(x) for x in k])
    # the vectorised form: one key, an array of counters
    out = gr.philox4x32_10((ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3]), (5, 7))
    for i in (0, 1, 17, 299):
        assert [int(o[i]) for o in out] == oracle_mod.philox([int(x) for x in ctr[i]], [5, 7])


def test_uniform_is_the_stated_function_of_seed_chain_sweep_node(oracle_mod):
    seed, chain, g, v = (0x9E3779B1 << 32) | 0x7F4A7C15, (1 << 32) + 3, 9, 5
    o = oracle_mod.philox([v, g, chain & 0xFFFFFFFF, chain >> 32], [seed & 0xFFFFFFFF, (seed >> 32) ^ gr.KEY_TAG])
    U = (o[0] << 21) | (o[1] >> 11)
    assert gr.uniform(seed, np.array([chain], dtype=np.uint64), g, v)[0] == U * 2.0 ** -53


@pytest.mark.parametrize("name", list(networks()))
def test_colouring_is_proper_on_the_moral_graph(name):
    m = networks()[name]
    col = gr.colouring(m)
    nb = gr.moral_neighbours(m)
    assert (col >= 0).all()
    for v in range(m.n):
        assert all(col[u] != col[v] for u in nb[v])
        assert all(any(col[u] == c for u in nb[v]) for c in range(int(col[v])))   # greedy: every smaller colour is taken
    if name == "star70":
        assert np.count_nonzero(col == col[1]) == 70    # one colour class with more slots than a wave has lanes


@pytest.mark.parametrize("name", list(networks()))
def test_library_plan_is_the_restatements_colouring(name, bnlib):
    """Engine.gibbs_plan() on an engine without a device: the planner's colouring is the restatement's, node for node."""
    from bayesiannetwork_amd import engine
    m = networks()[name]
    with engine.Engine(m, device=_lib.BN_DEVICE_HOST_ONLY) as e:
        plan = e.gibbs_plan()
        assert e.info("gibbs_eligible") == 1 and e.info("gibbs_colours") == plan["colours"]
        with pytest.raises(_lib.BnError) as ei:     # ... and no device, no run
            e.gibbs_run(np.full(m.n, -1, np.int32), 4, 2, seed=1)
        assert ei.value.code == _lib.BN_ERR_NO_DEVICE
    col = gr.colouring(m)
    assert np.array_equal(plan["colour"], col) and plan["colours"] == int(col.max()) + 1
    assert plan["max_class"] == int(np.bincount(col).max()) and 1 <= plan["sweeps_per_launch"] <= 256
    lanes = plan["threads"] // plan["chains_per_workgroup"]     # of a chain: the power of two, 8 .. 64, that covers the largest colour
    assert plan["threads"] == 256 and lanes == min(64, max(8, 1 << (plan["max_class"] - 1).bit_length())) and plan["lds_bytes"] <= 48 * 1024


def test_network_beyond_the_limits_is_refused_with_the_planners_reason(bnlib):
    from bayesiannetwork_amd import engine, from_parent_lists
    n = 4097
    wide = from_parent_lists([1] * n, [[] for _ in range(n)], [[1.0] for _ in range(n)])
    with engine.Engine(wide, device=_lib.BN_DEVICE_HOST_ONLY) as e:
        assert e.info("gibbs_eligible") == 0
        for call in (e.gibbs_plan, lambda: e.gibbs_run(np.full(n, -1, np.int32), 4, 2, seed=1)):
            with pytest.raises(_lib.BnError) as ei:
                call()
            assert ei.value.code == _lib.BN_ERR_STATE and "4097 nodes" in str(ei.value)


def test_split_runs_and_split_chains_add_up(oracle_mod):
    m = synth.random_dag(12, max_parents=3, window=6, k=3, seed=5)
    ev = ev_of(m, {2: 1, 9: 0})
    kw = dict(seed=77, burn_in=2, thin=3, chain_begin=(1 << 32) + 3, oracle=oracle_mod)
    whole = gr.run(m, ev, 9, 11, **kw)
    a = gr.run(m, ev, 9, 4, **kw)
    b = gr.run(m, ev, 9, 7, sweep_begin=4, init_states=a["states"], **kw)
    assert np.array_equal(b["states"], whole["states"])
    assert np.array_equal(a["counts"] + b["counts"], whole["counts"])
    assert a["kept"] + b["kept"] == whole["kept"] and a["stuck"] + b["stuck"] == whole["stuck"]
    kw2 = dict(kw, chain_begin=(1 << 32) + 3 + 5)
    lo, hi = gr.run(m, ev, 5, 11, **kw), gr.run(m, ev, 4, 11, **kw2)
    assert np.array_equal(np.concatenate([lo["states"], hi["states"]]), whole["states"])
    assert np.array_equal(lo["counts"] + hi["counts"], whole["counts"])
    assert whole["kept"] == 9 * 3 and int(whole["counts"].sum()) == whole["kept"] * m.n


def _exact(name, model, ev, bnlib):
    if name == "alarm":
        from bayesiannetwork_amd import Evidence, engine
        e = engine.Engine(model, device=_lib.BN_DEVICE_HOST_ONLY)
        try:
            plan = e.jt_plan()
        finally:
            e.close()
        return jr.Restatement(model, plan).run(Evidence.from_dict(model, {int(v): int(s) for v, s in enumerate(ev) if s >= 0}))[0]
    joint, pe = xr.einsum_marginals(model, ev)
    out = joint.copy()
    for v in range(model.n):
        out[model.node_off[v]:model.node_off[v + 1]] /= pe
    return out


def _statistics_case(name):
    if name == "grid3x3":
        m = synth.grid(3, 3, k=3)
        return m, ev_of(m, {1: 2, 8: 0})
    if name == "dag12":
        m = synth.random_dag(12, max_parents=3, window=6, k=3, seed=5)
        return m, ev_of(m, {2: 1, 9: 0})
    m = jr.alarm()
    return m, np.asarray(jr.ev_state_of(m, jr.hard_evidence(m, 0.1, 3)), dtype=np.int32)


@pytest.mark.parametrize("name", ["grid3x3", "dag12", "alarm"])
def test_final_states_follow_the_exact_posterior(name, oracle_mod, bnlib):
    """The final state of each of 4 096 chains after 32 sweeps: 4 096 independent draws.  Every state frequency lies within
    5 standard errors, 5 sqrt(max(p (1 - p), 1e-6) / 4096), of the exact posterior (the bound is the binomial's, not tuned:
    about a hundred comparisons at 5 sigma fail by chance less than once in 10^4 runs)."""
    m, ev = _statistics_case(name)
    exact = _exact(name, m, ev, bnlib)
    r = gr.run(m, ev, CHAINS, SWEEPS, seed=20261, oracle=oracle_mod)
    freq = gr.frequencies(m, r["states"])
    bound = 5.0 * np.sqrt(np.maximum(exact * (1.0 - exact), 1e-6) / CHAINS)
    dev = np.abs(freq - exact) / (bound / 5.0)
    print(f"{name}: worst deviation {dev.max():.2f} standard errors over {exact.size} frequencies, stuck {r['stuck']}")
    assert (np.abs(freq - exact) <= bound).all(), f"worst deviation {dev.max():.2f} standard errors"


def test_stuck_updates_on_pearl_and_the_posterior_all_the_same(oracle_mod):
    """Pearl's network holds zeros.  With W = 1 and H = 0 observed, a forward start with S = 1 leaves R no state: R = 0
    contradicts W = 1 (P(W = 1 | R = 0) = 0) and R = 1 contradicts H = 0 (P(H = 0 | R = 1, S = 1) = 0), so R's first update
    finds T = 0 and keeps its state; S then moves to 0 sooner or later and R is free again.  (H = 0 alone never sticks: R = 0
    always has weight.)  The restatement reports such updates.  A chain that starts at R = 0, S = 1 leaves that corner with
    probability 0.1 per sweep (S's conditional there is its prior), so 32 sweeps leave 0.9^32 = 3 % of those chains behind
    and 256 sweeps none (0.9^256 x 4096 < 1e-8): by then every chain sits on the posterior, which is the one point R = 1,
    S = 0."""
    m = synth.pearl()
    ev = ev_of(m, PEARL_STUCK_EVIDENCE)
    r = gr.run(m, ev, CHAINS, 256, seed=5, oracle=oracle_mod)
    assert r["stuck"] > 0
    exact = _exact("pearl", m, ev, None)
    assert np.array_equal(exact, [0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0])
    assert np.array_equal(gr.frequencies(m, r["states"]), exact)
    # ... and the count of stuck updates is the chains' own: none once S has moved, so a second run from there reports none
    again = gr.run(m, ev, CHAINS, 4, seed=5, sweep_begin=256, init_states=r["states"])
    assert again["stuck"] == 0
