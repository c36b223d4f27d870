"""Every reachable cell of the sampler family (tests/sampler_cases.py: CASES, CELLS) on the GPU, against the oracle bit for bit.

Sampled states, draw and acceptance counts are integer work: equal.  Weights agree to 1e-12 relative and weighted histograms to 1e-9
(the order of the fp64 atomics), unit-weight histograms exactly -- the tolerances of tests/test_lw_gpu.py, for the same reasons.
The kernel that ran is the one `classify` names (bn_get_info "lw_last_sample_kernel" / "lw_last_hist_kernel").
One engine at a time; nothing is retried."""
import numpy as np
import pytest

from sampler_cases import BLOCK, CASES, kahn_min_order, kernel_codes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine(bnlib):
    from bayesiannetwork_amd.engine import Engine
    return Engine


def _check_lw(model, ev, want, hist, states, weights):
    assert (states < model.k[None, :]).all(), "a state outside the node's arity"
    bad = np.argwhere(states != want["states"])
    assert bad.size == 0, f"{bad.shape[0]} states differ; first (sample, node) {bad[0].tolist()}: got {states[tuple(bad[0])]}, want {want['states'][tuple(bad[0])]}"
    assert np.allclose(weights, want["weights"], rtol=1e-12, atol=0)
    assert np.allclose(hist, want["hist"], rtol=1e-9, atol=1e-12)
    if (ev < 0).all():   # unit weights: histograms are integer counts, exact in fp64
        assert np.array_equal(hist, want["hist"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_bit_for_bit(Engine, oracle_mod, monkeypatch, case):
    monkeypatch.setenv("BN_LW_SMALL", "1" if case.small_env else "0")
    m, ev = case.model, case.ev_state
    topo = kahn_min_order(m)
    ns, seed, begin = case.n_samples, case.seed, case.sample_begin
    want = oracle_mod.lw_run(m, ev, ns, seed=seed, s_begin=begin, topo=topo, states_cap=ns)
    rs_calls = case.rs_params()
    rs_got = []
    with Engine(m) as eng:
        hist = eng.lw_run(ev, ns, seed=seed, sample_begin=begin)
        lw_codes = (eng.info("lw_last_sample_kernel"), eng.info("lw_last_hist_kernel"))
        states, weights = eng.lw_states(ns)
        for n_accept, max_draw in rs_calls:
            got = eng.rs_run(ev, n_accept, seed=seed, max_draw=max_draw, sample_begin=begin)
            rs_got.append((got, (eng.info("lw_last_sample_kernel"), eng.info("lw_last_hist_kernel"))))
    assert lw_codes == kernel_codes(m, ev, "lw", case.lw_run_args(), case.small_env)
    _check_lw(m, ev, want, hist, states, weights)
    for (n_accept, max_draw), ((counts, drawn, accepted), codes) in zip(rs_calls, rs_got):
        wc, wd, wa = oracle_mod.rs_run(m, ev, n_accept, seed=seed, max_draw=max_draw, s_begin=begin, topo=topo)
        assert (drawn, accepted) == (wd, wa)
        assert np.array_equal(counts, wc)
        assert (np.add.reduceat(counts, m.node_off[:-1]) == accepted).all()
        assert codes == kernel_codes(m, ev, "rs", dict(seed=seed, sample_begin=begin, n_accept=n_accept, max_draw=max_draw), case.small_env)
    (_, d1, a1), (_, d2, a2) = rs_got[0][0], rs_got[1][0]
    assert d2 == rs_calls[1][1] and a2 < rs_calls[1][0], "the second call was to stop at max_draw"
    if a1 == rs_calls[0][0]:
        assert d1 % BLOCK and d1 < rs_calls[0][1], "the first call was to stop at an acceptance inside a block"
    else:   # (evidence that is never, or hardly ever, met)
        assert d1 == rs_calls[0][1]
    case.drop_model()


def test_three_batches_on_the_generic_kernel(Engine, oracle_mod):
    """One bn_lw_run of more samples than the state matrix holds (bn_lw.cpp lw_prepare: 32 GiB / n rounded down to 1 024 samples, at
    most 16 384 x 1 024) on the generic kernel: three batches.  The call equals the sum of calls over windows that fit one batch,
    and a 4 096-sample window laid across the first batch boundary, run alone, equals the oracle."""
    from bayesiannetwork_amd import synth
    d = synth.random_dag(10000, 4, 64, [2, 3, 5], seed=1)
    ev = synth.random_evidence(d, 0.01, seed=7).hard_states(d)
    topo = kahn_min_order(d)
    batch = min((32 << 30) // d.n // BLOCK * BLOCK, 16384 * BLOCK)
    n_all, seed = 7_000_000, 5
    assert 2 * batch < n_all <= 3 * batch
    windows = [(0, 3_000_000), (3_000_000, 3_000_000), (6_000_000, 1_000_000)]
    assert all(cnt <= batch for _, cnt in windows)
    lo, cnt = batch - 2048, 4096
    want = oracle_mod.lw_run(d, ev, cnt, seed=seed, s_begin=lo, topo=topo, states_cap=cnt)
    with Engine(d) as eng:
        whole = eng.lw_run(ev, n_all, seed=seed)
        codes = (eng.info("lw_last_sample_kernel"), eng.info("lw_last_hist_kernel"))
        parts = sum(eng.lw_run(ev, c, seed=seed, sample_begin=b) for b, c in windows)
        sub = eng.lw_run(ev, cnt, seed=seed, sample_begin=lo)
        states, weights = eng.lw_states(cnt)
    assert codes == (16 + 4 + 2, 8)
    assert np.allclose(whole, parts, rtol=1e-9, atol=1e-300)
    _check_lw(d, ev, want, sub, states, weights)


@pytest.mark.parametrize("small", ["1", "0"])
def test_states_of_a_run_smaller_than_an_earlier_one(Engine, oracle_mod, monkeypatch, small):
    """The state matrix keeps the row stride of the largest call: bn_lw_states after a smaller one reads the right rows, through
    both transposes (two bits per state, one byte per state)."""
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_LW_SMALL", small)
    d = synth.random_dag(70, 3, 16, [2, 3, 4], seed=12)
    ev = synth.random_evidence(d, 0.05, seed=3).hard_states(d)
    topo = kahn_min_order(d)
    with Engine(d) as eng:
        eng.lw_run(ev, 9000, seed=8)
        assert eng.info("lw_small") == int(small == "1")
        hist = eng.lw_run(ev, 700, seed=8, sample_begin=4321)
        states, weights = eng.lw_states(700)
        c, drawn, acc = eng.rs_run(ev, 20, seed=8, max_draw=3000, sample_begin=11)
    _check_lw(d, ev, oracle_mod.lw_run(d, ev, 700, seed=8, s_begin=4321, topo=topo, states_cap=700), hist, states, weights)
    wc, wd, wa = oracle_mod.rs_run(d, ev, 20, seed=8, max_draw=3000, s_begin=11, topo=topo)
    assert (drawn, acc) == (wd, wa) and np.array_equal(c, wc)
