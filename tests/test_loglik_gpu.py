"""Log-likelihood scores on the GPU (bn_score_* of include/bn_mi355x.h, bayesiannetwork_amd.evaluation) against the
restatement in tests/loglik_refs.py.  The device takes no logarithm and adds in a stated order, so the row sums, the
family counts and the node sums are compared BIT FOR BIT; order-free yardsticks (math.fsum, the entropies of
bn_info_entropy, the reference's own loop) are compared to bounds built from the terms themselves:
gamma_m x sum |terms|, gamma_m = m u / (1 - m u), u = 2^-53 (no fixed tolerance anywhere)."""
import math
import os

import numpy as np
import pytest

import exact_refs
import loglik_refs as R
from bayesiannetwork_amd import _lib, synth
from bayesiannetwork_amd.dsc import load_dsc
from pattern_refs import random_patterns

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_COUNTS = [1, 63, 64, 65, 255, 256, 257, 4097]   # lane, wave and tile edges, the table's padding to 64
NODE_COUNTS = [1, 255, 256, 257, 513, 1025]             # segment edges
COUNTS = {"one": lambda r, P: np.ones(P, np.uint64),
          "127": lambda r, P: np.full(P, 127, np.uint64),
          "2^31": lambda r, P: np.full(P, 1 << 31, np.uint64),
          "2^40": lambda r, P: np.full(P, 1 << 40, np.uint64),
          "mixed": lambda r, P: r.choice(np.array([1, 127, 128, (1 << 31) - 1, 1 << 31, 1 << 40], np.uint64), P)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def alarm():
    return load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]


def edge_network(zero_frac=0.0, seed=1):
    """Arities 1, 2, 3, 5, 17, 255 mixed; nodes with 0, 1, 2, 5, 8 and 16 parents; tables of 1 to 131 072 entries, some
    above the counting kernel's 4 096-entry LDS limit."""
    ks = [2] * 16 + [3, 5, 1, 17, 255]                       # 0..15 binary roots; 16: k 3, 17: k 5, 18: k 1, 19: k 17, 20: k 255 (roots)
    parents = [[] for _ in ks]
    ks += [2, 3, 5, 255, 17, 1, 2, 3]
    parents += [list(range(16)),                             # 21: 16 parents, 2^16 x 2 entries
                list(range(8)),                              # 22: 8 parents, k 3
                [0, 16, 17, 18, 19],                         # 23: 5 parents of arities 2, 3, 5, 1, 17, k 5
                [19],                                        # 24: k 255 under a k 17 parent: 4 335 entries
                [20],                                        # 25: k 17 under a k 255 parent
                [1, 17],                                     # 26: k 1 with two parents
                [18],                                        # 27: a parent of arity 1
                [20, 24]]                                    # 28: two k 255 parents: 195 075 entries
    return exact_refs._model(ks, parents, np.random.default_rng(seed), zero_frac=zero_frac, name=f"edges_z{zero_frac}")


def mixed_dag(n, seed=3, zero_frac=0.0):
    base = synth.random_dag(n, 3, 16, [2, 3, 5, 1, 2, 17, 3, 2], seed=seed)
    if zero_frac == 0.0:
        return base
    parents = [list(base.parents(v)) for v in range(n)]
    return exact_refs._model([int(x) for x in base.k], parents, np.random.default_rng(seed), zero_frac=zero_frac, name=f"dag{n}_z")


def selections(n):
    last_seg = list(range((n - 1) // 256 * 256, n))
    return {"all": None, "one": [n // 2], "every other": list(range(0, n, 2)), "last segment": last_seg,
            "decreasing": list(range(n - 1, -1, -3))}


def engine_and_table(model, pats, counts=None):
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import InfoTable
    counts = np.ones(len(pats), np.uint64) if counts is None else counts
    return Engine(model, device=0), InfoTable(pats, counts, model.k, device=0)


# ---- 1. the log table --------------------------------------------------------------------------

def test_log_table_is_math_log_bit_for_bit_and_follows_reload(bnlib):
    from bayesiannetwork_amd import log_cpt, log_likelihood_nodes, log_likelihood_rows
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import InfoTable
    rng = np.random.default_rng(2)
    for model in (alarm(), edge_network(0.3), mixed_dag(300, zero_frac=0.2), synth.grid(12, 12, 3, seed=4)):
        pats = random_patterns(model.k, 500, seed=6)
        with Engine(model, device=0) as eng, InfoTable(pats, np.ones(500, np.uint64), model.k, device=0) as t:
            L = log_cpt(eng)
            assert same_bits(L, R.log_table(model))
            assert np.array_equal(np.isneginf(L), model.cpt == 0.0) and not np.isnan(L).any()
            before = log_likelihood_rows(eng, t)
            cpt = model.cpt.copy()
            for v in range(model.n):
                rows = int(model.cpt_off[v + 1] - model.cpt_off[v]) // int(model.k[v])
                cpt[model.cpt_off[v]:model.cpt_off[v + 1]] = exact_refs._random_table(rng, rows, int(model.k[v]), 0.0).reshape(-1)
            eng.reload_cpt(cpt)
            assert same_bits(log_cpt(eng), R.log_table(eng.model))
            after, after_nodes = log_likelihood_rows(eng, t), log_likelihood_nodes(eng, t)
            assert not same_bits(before, after)                                   # the old scores are gone
            with Engine(eng.model, device=0) as fresh:                            # ... and the new ones are a fresh engine's
                assert same_bits(after, log_likelihood_rows(fresh, t)) and same_bits(after_nodes, log_likelihood_nodes(fresh, t))
            assert same_bits(after, R.rows_ref(eng.model, pats))


# ---- 2. rows, bit-exact ------------------------------------------------------------------------

def check_rows(model, pattern_counts, seed=0):
    from bayesiannetwork_amd import log_likelihood_rows
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import InfoTable
    L = R.log_table(model)
    with Engine(model, device=0) as eng:
        for P in pattern_counts:
            pats = random_patterns(model.k, P, seed=seed + P)
            with InfoTable(pats, np.ones(P, np.uint64), model.k, device=0) as t:
                for name, sel in selections(model.n).items():
                    got = log_likelihood_rows(eng, t, sel)
                    want = R.rows_ref(model, pats, sel, L)
                    assert got.shape == (P,) and same_bits(got, want), (model.name, P, name)
                    if sel is not None and len(sel) > 1:   # the order of the list does not matter
                        shuffled = np.random.default_rng(P).permutation(sel)
                        assert same_bits(log_likelihood_rows(eng, t, shuffled), want), (model.name, P, name, "shuffled")


@pytest.mark.parametrize("net", ["alarm", "edges", "grid"])
def test_rows_bit_exact_on_named_networks(bnlib, net):
    model = {"alarm": alarm, "edges": edge_network, "grid": lambda: synth.grid(9, 13, 3, seed=5)}[net]()
    check_rows(model, PATTERN_COUNTS)


@pytest.mark.parametrize("n", NODE_COUNTS)
def test_rows_bit_exact_at_segment_edges(bnlib, n):
    check_rows(mixed_dag(n, seed=n), PATTERN_COUNTS, seed=n)


# ---- 3. a row's score is a function of the row -------------------------------------------------

def test_rows_are_a_function_of_the_row(bnlib):
    from bayesiannetwork_amd import log_likelihood_rows
    from bayesiannetwork_amd.evaluation import InfoTable
    for model in (edge_network(), mixed_dag(513)):
        pats = random_patterns(model.k, 4097, seed=9)
        perm = np.random.default_rng(1).permutation(4097)
        eng, t = engine_and_table(model, pats)
        with eng, t, InfoTable(pats[perm], np.ones(4097, np.uint64), model.k, device=0) as tp:
            ll = log_likelihood_rows(eng, t)
            assert same_bits(log_likelihood_rows(eng, tp), ll[perm])
            for p in (0, 1, 63, 64, 2048, 4095, 4096):
                with InfoTable(pats[p:p + 1], np.ones(1, np.uint64), model.k, device=0) as one:
                    assert same_bits(log_likelihood_rows(eng, one), ll[p:p + 1]), p


# ---- 4. zeros ----------------------------------------------------------------------------------

def test_zero_entries_give_minus_infinity_and_never_nan(bnlib):
    from bayesiannetwork_amd import log_likelihood_nodes, log_likelihood_rows
    for model in (exact_refs.polytree(200, arities=(2, 3, 4), zero_frac=0.3, seed=7), exact_refs.chain(300, k=3, seed=2, zero_frac=0.4),
                  edge_network(0.3), mixed_dag(257, zero_frac=0.25)):
        rng = np.random.default_rng(31)
        possible = np.array([exact_refs.forward_sample(model, rng) for _ in range(100)], dtype=np.uint8)   # rows the network can produce
        pats = np.concatenate([random_patterns(model.k, 900, seed=12), possible])[rng.permutation(1000)]
        q = R.entry_index(model, pats)
        hits = (model.cpt[q] == 0.0).any(axis=1)
        assert hits.any() and (~hits).sum() >= 100
        eng, t = engine_and_table(model, pats)
        with eng, t:
            ll = log_likelihood_rows(eng, t)
            assert not np.isnan(ll).any()
            assert np.array_equal(np.isneginf(ll), hits)
            assert same_bits(ll, R.rows_ref(model, pats))            # ... so the other rows are unaffected
            nodes, N = log_likelihood_nodes(eng, t, counts=True)
            assert not np.isnan(nodes).any()                        # unseen zero entries: skipped, not 0 x -inf
            assert same_bits(nodes, R.nodes_ref(model, N))
            seen_zero = np.array([((model.cpt[model.cpt_off[v]:model.cpt_off[v + 1]] == 0.0) & (N[model.cpt_off[v]:model.cpt_off[v + 1]] != 0)).any()
                                  for v in range(model.n)])
            assert np.array_equal(np.isneginf(nodes), seen_zero)


# ---- 5. family counts --------------------------------------------------------------------------

@pytest.mark.parametrize("counts", sorted(COUNTS))
def test_family_counts_exact(bnlib, counts):
    from bayesiannetwork_amd import log_likelihood_nodes
    assert (np.diff(edge_network().cpt_off) > 4096).sum() >= 3 and (np.diff(edge_network().cpt_off) <= 4096).any()   # both sides of the counter's LDS / global switch
    for model, P in ((edge_network(), 3000), (alarm(), 4097), (mixed_dag(257), 65)):
        rng = np.random.default_rng(P)
        pats = random_patterns(model.k, P, seed=13)
        c = COUNTS[counts](rng, P)
        eng, t = engine_and_table(model, pats, c)
        with eng, t:
            for splits in (0, 1, 7):                                 # integer atomics: the split cannot matter
                eng.set_option("score_splits", splits)
                _, N = log_likelihood_nodes(eng, t, counts=True)
                assert N.dtype == np.uint64 and np.array_equal(N, R.family_counts_ref(model, pats, c)), (model.name, splits)


# ---- 6. node sums ------------------------------------------------------------------------------

@pytest.mark.parametrize("counts", ["one", "mixed"])
def test_node_sums_bit_exact_permutation_and_split_invariant(bnlib, counts):
    from bayesiannetwork_amd import log_likelihood_nodes
    from bayesiannetwork_amd.evaluation import InfoTable
    for model in (alarm(), edge_network(), mixed_dag(513), synth.grid(9, 13, 3, seed=5)):
        P = 3000
        rng = np.random.default_rng(17)
        pats = random_patterns(model.k, P, seed=14)
        c = COUNTS[counts](rng, P)
        L = R.log_table(model)
        eng, t = engine_and_table(model, pats, c)
        with eng, t:
            ll, N = log_likelihood_nodes(eng, t, counts=True)
            assert same_bits(ll, R.nodes_ref(model, N, L)), model.name
            perm = rng.permutation(P)
            with InfoTable(pats[perm], c[perm], model.k, device=0) as tp:
                assert same_bits(log_likelihood_nodes(eng, tp), ll)
            # every pattern's count split over two identical rows
            half = c // np.uint64(2)
            keep = half > 0
            pats2 = np.concatenate([pats, pats[keep]])
            c2 = np.concatenate([c - half, half[keep]])
            with InfoTable(pats2, c2, model.k, device=0) as ts:
                assert same_bits(log_likelihood_nodes(eng, ts), ll)
            # against math.fsum: m = non-zero terms + 1 (the double(N) conversion), from the terms themselves
            for v in range(model.n):
                terms = R.node_terms(model, N, L, v)
                nz = terms[terms != 0]
                bound = R.gamma(len(nz) + 1) * math.fsum(np.abs(nz).tolist())
                assert abs(ll[v] - R.exact_total(nz)) <= bound, (model.name, v, ll[v], R.exact_total(nz), bound)


# ---- 7. the two routes agree -------------------------------------------------------------------

def test_rows_weighted_by_counts_equal_the_node_sums(bnlib):
    from bayesiannetwork_amd import log_likelihood_nodes, log_likelihood_rows
    for model in (alarm(), mixed_dag(513), synth.grid(9, 13, 3, seed=5)):
        P = 4097
        rng = np.random.default_rng(19)
        pats = random_patterns(model.k, P, seed=15)
        c = rng.integers(1, 1 << 20, P).astype(np.uint64)
        L = R.log_table(model)
        eng, t = engine_and_table(model, pats, c)
        with eng, t:
            rows = log_likelihood_rows(eng, t)
            nodes, N = log_likelihood_nodes(eng, t, counts=True)
        by_rows = math.fsum(float(w) * x for w, x in zip(c.tolist(), rows.tolist()))
        by_nodes = math.fsum(nodes.tolist())
        # rows side: each row sum carries <= n - 1 roundings, the product with the count one more; nodes side: likelihood_bound
        rows_bound = R.gamma(model.n + 1) * math.fsum(float(w) * math.fsum(np.abs(L[q]).tolist()) for w, q in zip(c.tolist(), R.entry_index(model, pats)))
        bound = rows_bound + R.likelihood_bound(model, N, L)
        print(f"{model.name}: by rows {by_rows!r} by nodes {by_nodes!r} |diff| {abs(by_rows - by_nodes):.3e} bound {bound:.3e}")
        assert abs(by_rows - by_nodes) <= bound


# ---- 8. against the entropies -------------------------------------------------------------------

def test_fitted_network_likelihood_equals_conditional_entropies(bnlib):
    """For maximum-likelihood CPTs (fit_cpt of the same table), -sum_v ll_node[v] / (N ln 2) = sum_v H(v, Pa(v)) - H(Pa(v)).

    The bound, derived (not observed).  Counts are small, so N_q, N_row and N convert exactly.  Entropy side, per set S:
    a term is fl(p x fl(log2 fl(c / N))); p carries one rounding (relative u), which moves log2 p by at most u / ln 2
    absolutely; log2 itself is taken as correct to 2 ulp, the product adds one rounding: |error of a term| <= p (4 u |log2 p|
    + 1.45 u), and adding `cells` terms in any order costs gamma_cells x sum |terms|.  With sum p = 1 that is at most
    gamma_(cells + 4) x (H(S) + 1.45).  Likelihood side, per node: theta = fl(N_q / N_row) (one rounding, moves log theta by
    at most u absolutely), libm's log within 1 ulp, the product one rounding, the sum gamma_m: at most
    gamma_(m + 3) x (sum N_q |L_q| + N_v) / (N ln 2), N_v = N the samples counted at the node.  `cells` is the product of
    the set's arities, m the non-zero terms of the node."""
    from bayesiannetwork_amd import log_likelihood_nodes
    from bayesiannetwork_amd.engine import Engine, fit_cpt
    from bayesiannetwork_amd.evaluation import InfoTable
    for structure in (alarm(), mixed_dag(120, seed=8), synth.grid(6, 7, 3, seed=5)):
        P = 3000
        rng = np.random.default_rng(23)
        pats = random_patterns(structure.k, P, seed=16)
        c = rng.integers(1, 100, P).astype(np.uint64)
        total = int(c.sum())
        fitted = type(structure)(structure.k, structure.in_ptr, structure.in_idx, structure.cpt_off, fit_cpt(structure, pats, c, device=0),
                                 name=structure.name + "_fitted")
        L = R.log_table(fitted)
        with Engine(fitted, device=0) as eng, InfoTable(pats, c, fitted.k, device=0) as t:
            ll, N = log_likelihood_nodes(eng, t, counts=True)
            assert np.isfinite(ll).all()
            lhs, rhs, bound = [], [], 0.0
            for v in range(fitted.n):
                pa = [int(u) for u in fitted.parents(v)]
                h_joint = t.entropy(pa + [v])
                h_pa = t.entropy(pa) if pa else 0.0
                rhs += [h_joint, -h_pa]
                lhs.append(-ll[v] / (total * math.log(2.0)))
                cells_pa = math.prod(int(fitted.k[u]) for u in pa)
                terms = R.node_terms(fitted, N, L, v)
                m = int((terms != 0).sum())
                bound += R.gamma(cells_pa * int(fitted.k[v]) + 4) * (h_joint + 1.45) + (R.gamma(cells_pa + 4) * (h_pa + 1.45) if pa else 0.0)
                bound += R.gamma(m + 3) * (math.fsum(np.abs(terms).tolist()) + total) / (total * math.log(2.0))
            a, b = math.fsum(lhs), math.fsum(rhs)
            bound += 4 * 2.0 ** -53 * (abs(a) + math.fsum(abs(x) for x in rhs))   # the divisions and the two fsum roundings
            print(f"{fitted.name}: -ll / (N ln 2) = {a!r}, sum of conditional entropies = {b!r}, |diff| {abs(a - b):.3e}, bound {bound:.3e}")
            assert abs(a - b) <= bound


# ---- 9. AIC / MDL (Python side; the C++ functors: tests/test_cpp_scores.py) ---------------------

def test_aic_mdl_against_the_reference_loop(bnlib):
    from bayesiannetwork_amd import AIC, MDL, parameters
    from bayesiannetwork_amd.engine import Engine, Sampler
    from bayesiannetwork_amd.evaluation import InfoTable
    model = alarm()
    by_hand = sum((int(model.k[v]) - 1) * math.prod(int(model.k[u]) for u in model.parents(v)) for v in range(model.n))
    rng = np.random.default_rng(29)
    table = {}
    for _ in range(500):
        key = tuple(int(x) for x in exact_refs.forward_sample(model, rng))
        table[key] = table.get(key, 0) + int(rng.integers(1, 1000))
    size = sum(table.values())
    pats = np.array(list(table.keys()), dtype=np.uint8)
    cnts = np.array(list(table.values()), dtype=np.uint64)
    L = R.log_table(model)
    N = R.family_counts_ref(model, pats, cnts)
    sampler = Sampler()
    sampler.load_sample(table)
    subset = [30, 2, 17, 5]
    with Engine(model, device=0) as eng, InfoTable(pats, cnts, model.k, device=0) as t:
        assert parameters(eng) == parameters(model) == by_hand
        for nodes in (None, subset):
            sel = range(model.n) if nodes is None else nodes
            mags = math.fsum(abs(x) for v in sel for x in R.node_terms(model, N, L, v).tolist())
            m = sum(int((R.node_terms(model, N, L, v) != 0).sum()) for v in sel)
            for functor, ref, extra in ((AIC, R.reference_aic, float(by_hand)), (MDL, R.reference_mdl, by_hand * (math.log2(size) / 2))):
                want = ref(model, table, nodes)
                bound = R.gamma(m + 2) * (mags + abs(extra))
                got_table, got_sampler, got_model = functor(t)(eng, nodes), functor(sampler, device=0)(eng, nodes), functor(t)(model, nodes)
                print(f"{functor.__name__} nodes={nodes}: got {got_table!r} reference {want!r} |diff| {abs(got_table - want):.3e} bound {bound:.3e}")
                assert abs(got_table - want) <= bound
                assert got_model == got_table                     # an engine built from the model: the same bits
                assert abs(got_sampler - want) <= bound           # (the sampler's table has its own row order: same node sums)
                assert got_sampler == got_table
        # a subset keeps the whole graph's parameters (aic.hpp:23-24)
        assert AIC(t)(eng, []) == float(by_hand)
    with pytest.raises(RuntimeError, match="Sampling is not finished yet."):
        MDL(Sampler())(model)


# ---- 10. errors --------------------------------------------------------------------------------

def test_errors_name_their_cause_and_leave_the_engine_usable(bnlib):
    from bayesiannetwork_amd import log_likelihood_nodes, log_likelihood_rows
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import InfoTable
    model = mixed_dag(300)
    pats = random_patterns(model.k, 100, seed=3)
    ones = np.ones(100, np.uint64)
    out, outn = np.zeros(100), np.zeros(model.n)
    f64 = lambda a: a.ctypes.data_as(_lib.f64p)       # noqa: E731
    i32 = lambda a: a.ctypes.data_as(_lib.i32p)       # noqa: E731

    def expect(rc, code, text):
        assert rc == code and text in bnlib.bn_last_error().decode(), (rc, bnlib.bn_last_error())

    other_k = model.k.copy()
    other_k[7] += 1
    with Engine(model, device=0) as eng, InfoTable(pats, ones, model.k, device=0) as t, \
            InfoTable(pats[:, :-1], ones, model.k[:-1], device=0) as narrow, InfoTable(pats, ones, other_k, device=0) as wider:
        expect(bnlib.bn_score_rows(None, t._h, 0, None, f64(out)), _lib.BN_ERR_ARG, "null")
        expect(bnlib.bn_score_rows(eng._h, None, 0, None, f64(out)), _lib.BN_ERR_ARG, "null")
        expect(bnlib.bn_score_rows(eng._h, t._h, 0, None, None), _lib.BN_ERR_ARG, "null")
        expect(bnlib.bn_score_nodes(eng._h, t._h, None, None), _lib.BN_ERR_ARG, "null")
        expect(bnlib.bn_score_nodes(None, t._h, f64(outn), None), _lib.BN_ERR_ARG, "null")
        expect(bnlib.bn_score_log_cpt(eng._h, None), _lib.BN_ERR_ARG, "null")
        expect(bnlib.bn_score_rows(eng._h, narrow._h, 0, None, f64(out)), _lib.BN_ERR_ARG, "columns")
        expect(bnlib.bn_score_nodes(eng._h, narrow._h, f64(outn), None), _lib.BN_ERR_ARG, "columns")
        expect(bnlib.bn_score_rows(eng._h, wider._h, 0, None, f64(out)), _lib.BN_ERR_ARG, "arity of column 7")
        expect(bnlib.bn_score_nodes(eng._h, wider._h, f64(outn), None), _lib.BN_ERR_ARG, "arity of column 7")
        expect(bnlib.bn_score_rows(eng._h, t._h, 2, i32(np.array([3, 3], np.int32)), f64(out)), _lib.BN_ERR_ARG, "listed twice")
        expect(bnlib.bn_score_rows(eng._h, t._h, 1, i32(np.array([model.n], np.int32)), f64(out)), _lib.BN_ERR_ARG, "out of range")
        expect(bnlib.bn_score_rows(eng._h, t._h, 1, i32(np.array([-1], np.int32)), f64(out)), _lib.BN_ERR_ARG, "out of range")
        with Engine(model, device=_lib.BN_DEVICE_HOST_ONLY) as host:
            expect(bnlib.bn_score_rows(host._h, t._h, 0, None, f64(out)), _lib.BN_ERR_NO_DEVICE, "host-only")
            expect(bnlib.bn_score_nodes(host._h, t._h, f64(outn), None), _lib.BN_ERR_NO_DEVICE, "host-only")
        with Engine(model, device=0, rank=0, nranks=2) as shard:
            expect(bnlib.bn_score_rows(shard._h, t._h, 0, None, f64(out)), _lib.BN_ERR_STATE, "sharded")
            expect(bnlib.bn_score_nodes(shard._h, t._h, f64(outn), None), _lib.BN_ERR_STATE, "sharded")
            expect(bnlib.bn_score_log_cpt(shard._h, f64(np.zeros(int(model.cpt_off[-1])))), _lib.BN_ERR_STATE, "sharded")
        try:
            import torch
            two = torch.cuda.device_count() > 1
        except Exception:  # noqa: BLE001
            two = False
        if two:   # (a box with one device cannot hold the pair)
            with InfoTable(pats, ones, model.k, device=1) as far:
                expect(bnlib.bn_score_rows(eng._h, far._h, 0, None, f64(out)), _lib.BN_ERR_ARG, "different devices")
        # after the errors the engine still scores correctly
        assert same_bits(log_likelihood_rows(eng, t), R.rows_ref(model, pats))
        ll, N = log_likelihood_nodes(eng, t, counts=True)
        assert same_bits(ll, R.nodes_ref(model, N)) and np.array_equal(N, R.family_counts_ref(model, pats, ones))
        assert same_bits(log_likelihood_rows(eng, t, []), np.zeros(100))     # nothing selected: the empty sum


# ---- 11. sampler round trip --------------------------------------------------------------------

def test_sampler_round_trip_on_pearl(bnlib):
    """LikelihoodWeighting.make_samples -> Sampler -> make_cpt -> MDL, end to end."""
    from bayesiannetwork_amd import MDL
    from bayesiannetwork_amd.engine import LikelihoodWeighting, Sampler
    pearl = synth.pearl()
    lw = LikelihoodWeighting(pearl, device=0, seed=7)
    patterns, _ = lw.make_samples(None, unit_size=20000, epsilon=0.01)
    lw.engine.close()
    sampler = Sampler()
    assert sampler.load_sample(patterns) and sampler.sampling_size() >= 20000
    fitted = type(pearl)(pearl.k, pearl.in_ptr, pearl.in_idx, pearl.cpt_off, pearl.cpt.copy(), name="pearl_fitted")
    assert sampler.make_cpt(fitted)
    score = MDL(sampler, device=0)(fitted)
    pats = np.array(list(patterns.keys()), dtype=np.uint8)
    cnts = np.array(list(patterns.values()), dtype=np.uint64)
    N = R.family_counts_ref(fitted, pats, cnts)
    likelihood = 0.0
    for x in R.nodes_ref(fitted, N).tolist():
        likelihood -= x
    want = likelihood + float(R.parameters_ref(fitted)) * (math.log2(float(sampler.sampling_size())) / 2)
    assert math.isfinite(score) and score == want
    ref = R.reference_mdl(fitted, patterns)
    bound = R.likelihood_bound(fitted, N, R.log_table(fitted)) + R.gamma(3) * abs(ref)
    print(f"pearl round trip: MDL {score!r} reference loop {ref!r} bound {bound:.3e}")
    assert abs(score - ref) <= bound
