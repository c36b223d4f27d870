"""The restatement of the Bayesian-Dirichlet scores (tests/bd_refs.py) checked on the CPU: lgamma_pos against libm and against
exact factorials, the bound B_bd under a logarithm moved by up to 3 ulp, and the margin condition that lets tests/test_bd_gpu.py
demand equal edges without leaving a decision out.

One decision class cannot meet the margin condition on ANY input: the full brute-force enumeration under BDeu.  BDeu is score
equivalent -- a -> b and b -> a have the same score in exact arithmetic -- and the enumeration compares every graph with the best so
far, so it always compares two equivalent graphs whose computed scores differ by rounding alone.  That is shown here, not assumed;
the GPU test therefore checks the full enumeration under BDeu bit for bit over the device's own terms and its final score within
the bounds, and demands equal edges of it under K2 (not score equivalent) and of the hint enumeration under both scores."""
import math

import numpy as np
import pytest

import anneal_refs as AR
import bd_refs as BD
import hc_refs as HR
import learning_refs as LR
import subset_refs as SS

U = BD.U


def M_of(x):
    return BD.lgamma_pos(x)[1]


def check_difference(a, N):
    got = BD.lgamma_pos(a + N)[0] - BD.lgamma_pos(a)[0]
    want = math.lgamma(a + N) - math.lgamma(a)
    bound = 16 * U * (M_of(a + N) + M_of(a))
    assert abs(got - want) <= bound, (a, N, got, want, abs(got - want) / bound)
    return abs(got - want) / (U * (M_of(a + N) + M_of(a)))


def test_lgamma_pos_stays_within_16u_of_libm():
    worst = 0.0
    for a in (1.0, 2.0, 255.0, 1.0 / 3.0, 0.5, 2.0 ** -40, 2.0 ** 20):
        for N in (1.0, 15.0, 16.0, 17.0, 2.0 ** 40):
            worst = max(worst, check_difference(a, N))
    for a, N in ((1.0, 15.0), (0.5, 15.5), (15.0, 1.0), (2.0 ** -60, 16.0)):   # a + N exactly 16 (the last: 16 after rounding)
        assert a + N == 16.0
        worst = max(worst, check_difference(a, N))
    rng = np.random.default_rng(20)
    for _ in range(20000):
        a = 10.0 ** rng.uniform(-7, 1)
        N = float(int(10.0 ** rng.uniform(0, 12)))
        worst = max(worst, check_difference(a, N))
    print(f"largest |lgamma_pos difference - libm| = {worst:.2f} u (M(a + N) + M(a)); allowed 16")
    assert struct_bits(BD.HALF_LOG_2PI) == 0x3FED67F1C864BEB4 and BD.HALF_LOG_2PI == 0.5 * math.log(2 * math.pi)


def struct_bits(x):
    return AR.bits(x)


def test_k2_terms_equal_the_log_of_exact_factorial_ratios():
    """K2: the family term is log of  prod_j [(kc - 1)! / (tot_j + kc - 1)! * prod_s N_js!]  -- big integers, then one logarithm each."""
    rng = np.random.default_rng(21)
    for kc, R in ((2, 1), (3, 4), (255, 2), (1, 3), (5, 7)):
        N = rng.integers(0, 2001, (R, kc)).astype(np.uint64)
        N[rng.integers(R)] = 0 if R > 1 else N[0]
        N[0, 0] = 2000
        t, sum_M, m = BD.bd_terms(N, kc, BD.K2S)
        num = den = 1
        for row in N.tolist():
            if sum(row) == 0:
                continue
            num *= math.factorial(kc - 1) * math.prod(math.factorial(x) for x in row)
            den *= math.factorial(sum(row) + kc - 1)
        want = math.log(num) - math.log(den)
        got = math.fsum(t.tolist())
        slack = 16 * U * sum_M + 4 * U * (math.log(num) + math.log(den))
        assert abs(got - want) <= slack, (kc, R, got, want)
        if kc == 1:
            assert got == 0.0 and m == 0


def test_a_logarithm_moved_by_three_ulp_stays_within_the_bound_on_every_family_of_the_gpu_tests():
    worst = 0.0
    cases = [(BD.SMALL_PATS, BD.SMALL_COUNTS, BD.SMALL_K, [(1, [0], [])], BD.SPECS)]
    for P, specs in BD.TERM_CASES:
        pats, counts = BD.term_table(P)
        cases.append((pats, counts, BD.KS, BD.GROUPS, specs))
    for pats, counts, ks, groups, specs in cases:
        for child, parents in BD.families_of(groups):
            N = LR.family_counts(pats, counts, ks, child, parents)
            for i, spec in enumerate(specs):
                plain, exact, bound = BD.bd_family(N, ks[child], spec)
                moved, _, _ = BD.bd_family(N, ks[child], spec, log=BD.PerturbedLog(1000 * child + i))
                assert abs(moved - plain) <= bound and abs(moved - exact) <= bound, (child, parents, spec, moved - plain, bound)
                if bound:
                    worst = max(worst, abs(moved - plain) / bound)
    print(f"largest |perturbed - plain| / B_bd: {worst:.3g}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
def test_every_learner_decision_has_a_margin_of_a_thousand_bounds(spec):
    model, table = BD.learner_input()
    bdt = BD.BDTable(table, spec)
    out = BD.run_searches(lambda start: BD.BDSearch(model.k, start, bdt.term, BD.MAX_PARENTS, record=True), bdt)
    margins = out["margins"]
    assert len(margins) > 100 and BD.margins_ok(margins), min(m / b for m, b in margins)
    print(f"{spec}: {len(margins)} decisions, smallest margin / bound {min(m / b for m, b in margins):.3g}")
    for name in ("greedy", "hint", "k2", "best"):
        L = out[name][2]
        assert sum(map(len, L.parents)) > 0, name
        assert AR.bits(L.score) == AR.bits(BD.likelihood_alone(L.ll)), name   # the "mdl over a total of 1" score IS the likelihood alone


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
def test_brute_force_margins_and_the_one_class_that_cannot_have_them(spec):
    model, table = BD.brute_input()
    bdt = BD.BDTable(table, spec)
    # the hint enumeration: literal, because child 1 reaches parent node 2
    L = BD.BDSearch(table.k, BD.BRUTE_HINT_START, bdt.term, BD.MAX_PARENTS)
    assert not L.decomposes(*BD.BRUTE_HINT)
    best, score, leaves = SS.literal_hint(L, *BD.BRUTE_HINT)
    margins = BD.leaf_margins(bdt, L.parents, L.score, leaves)
    assert len(margins) >= 16 and BD.margins_ok(margins), min(m / b for m, b in margins)
    assert L.brute_force_hint(*BD.BRUTE_HINT) == score and L.parents == best
    # the full enumeration
    L = BD.BDSearch(table.k, LR.empty_graph(table.n), bdt.term, BD.MAX_PARENTS)
    best, ev, leaves = SS.literal_brute_force(L, BD.BRUTE_VERTEXES)
    margins = BD.leaf_margins(bdt, L.parents, L._score(L.parents, BD.BRUTE_VERTEXES), leaves)
    assert L.brute_force(BD.BRUTE_VERTEXES) == ev and L.parents == best
    if spec.kind == 3:
        assert BD.margins_ok(margins), min(m / b for m, b in margins)
    else:
        # score equivalence: the reversal of a single edge is compared with it and differs by rounding alone
        a = BD.likelihood_alone([bdt.term(v, [0] if v == 1 else []) for v in range(table.n)])
        b = BD.likelihood_alone([bdt.term(v, [1] if v == 0 else []) for v in range(table.n)])
        assert abs(a - b) <= bdt.graph_bound([[], [0], [], [], []]) + bdt.graph_bound([[1], [], [], [], []])
        assert not BD.margins_ok(margins)


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
def test_the_literal_and_the_restated_chain_agree_under_the_likelihood_alone(spec):
    for name in ("n5_met", "n5_ref", "n33_dense_met"):
        inp, q, rule, t0, t1, rate, boltz, same, cap, chains, seed = BD.ANNEAL[name]
        _, table = AR.anneal_input(inp)
        pb = BD.BDProblem(table.k, q, BD.bd_term_fn(BD.BDTable(table, spec)), BD.ANNEAL_START.get(name))
        sched = AR.Schedule(t0, t1, rate, boltz, same, rule, cap)
        operated = 0
        for j in range(chains):
            lit, res = AR.literal_chain(pb, sched, seed, j), AR.restated_chain(pb, sched, seed, j)
            for key in ("eval", "proposals", "operated", "accepted", "flags", "masks", "trace"):
                assert lit[key] == res[key], (name, j, key)
            assert [tuple(e) for e in lit["edges"]] == [tuple(e) for e in res["edges"]]
            assert AR.exp_margin_ok(res["uphill"]), (name, j)
            operated += res["operated"]
        assert operated > 10 * chains, name


@pytest.mark.parametrize("spec", BD.LEARNER_SPECS, ids=repr)
def test_the_literal_and_the_restated_hc_run_agree_under_the_likelihood_alone(spec):
    for name in ("n5", "n33_nan_first", "n33_inf_sparse"):
        inp, q, alpha, runs, seed = BD.HC[name]
        _, table = AR.anneal_input(inp)
        pb = BD.BDProblem(table.k, q, BD.bd_term_fn(BD.BDTable(table, spec)))
        S = HR.similarity_matrix(BD.HC_SIMILARITY[name], table.n) if name in BD.HC_SIMILARITY else HR.host_mi(table)
        for j in range(min(runs, 8)):
            lit, res = HR.literal_run(pb, S, alpha, seed, j), HR.restated_run(pb, S, alpha, seed, j)
            for key in ("score", "merges", "masks", "flags"):
                a, b = lit[key], res[key]
                assert (HR.bits(a) == HR.bits(b) if key == "score" else a == b), (name, j, key)
            assert HR.pow_margin_ok(res["decisions"], alpha, res["exponents"]), (name, j)
