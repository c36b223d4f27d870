"""CPU checks of the sampler case list (tests/sampler_cases.py): the cases visit every reachable cell of the sampler family's code,
`relabel` preserves the joint, and the oracle the GPU is compared with (oracle/lw_oracle.c) is right at these edges -- checked
against a plain restatement of the reference's loops written here."""
import numpy as np
import pytest

import exact_refs as X
import sampler_cases as S
from sampler_cases import CASES, CELLS, kahn_min_order, relabel


@pytest.fixture(scope="module")
def cells_by_case():
    out = {}
    for c in CASES:
        out[c.name] = c.cells()
        c.drop_model()
    return out


def test_cases_visit_every_cell_and_no_other(cells_by_case):
    """Coverage is asserted, not hoped for: the union of classify() over CASES is the declared list."""
    seen = set().union(*cells_by_case.values())
    assert len(set(CELLS)) == len(CELLS)
    missing = sorted(set(CELLS) - seen)
    extra = sorted(seen - set(CELLS))
    assert not missing, f"cells no case visits any more: {missing}"
    assert not extra, f"cells visited but not declared in CELLS: {extra}"


@pytest.mark.parametrize("drop,cell", [("rows_2_24", "gen:rows:mul32"), ("hist_8_samples264141", "hist:hist<8>:segs=odd"),
                                       ("hist2_2_samples1024", "hist:hist2<2>:nvalid%range==0")])
def test_a_dropped_case_is_noticed(cells_by_case, drop, cell):
    """The only visitor of a cell cannot leave the list silently: without it the union no longer equals CELLS."""
    rest = set().union(*(cs for name, cs in cells_by_case.items() if name != drop))
    assert cell in cells_by_case[drop] and cell not in rest
    assert rest != set(CELLS)


def test_relabel_preserves_the_joint():
    m = S.net([3, 2, 4, 2, 1, 3, 2], [[], [0], [0, 1], [1, 2], [0, 3], [2, 3, 4], [0, 1, 3, 5]], 5, "seven")
    ev = S.ev_of(m, {3: 1, 5: 2})
    joint, pe = X.einsum_marginals(m, ev)
    for seed in (1, 2, 3):
        perm = S.scramble(m.n, seed)
        r = relabel(m, perm)
        r.validate()
        jr, per = X.einsum_marginals(r, S.relabel_states(ev, perm))
        assert np.isclose(per, pe, rtol=1e-13)
        for old in range(m.n):
            new = int(perm[old])
            assert np.allclose(jr[r.node_off[new]:r.node_off[new + 1]], joint[m.node_off[old]:m.node_off[old + 1]], rtol=1e-12, atol=0)
    # at least one of these permutations makes the visiting order differ from the identity (what the relabelled cases are for)
    assert any((kahn_min_order(relabel(m, S.scramble(m.n, s))) != np.arange(m.n)).any() for s in (1, 2, 3))


# ---- the oracle against a plain restatement of likelihood_weighting.hpp:122-193 and rejection_sampling.hpp:70-111 ----------------------

def _pick(u, row):
    """make_random_by_weight (:177-193): first i with total_{i-1} <= u < total_i, totals added left to right in fp64; else the last."""
    total = 0.0
    for i, x in enumerate(row):
        old = total
        total = total + float(x)
        if old <= u and u < total:
            return i
    return len(row) - 1


def _draw(model, topo, ev_state, seed, s, oracle, clamp):
    """One sample: (states, weight).  clamp: likelihood weighting (evidence nodes take their state, the weight their entry);
    otherwise every node is drawn (rejection sampling)."""
    state = [0] * model.n
    w = 1.0
    for t, v in enumerate(topo):
        v = int(v)
        u = oracle.lw_uniform(seed, s, t)
        row = 0
        for p in model.parents(v):
            row = row * int(model.k[p]) + state[int(p)]
        kv = int(model.k[v])
        base = int(model.cpt_off[v]) + row * kv
        r = model.cpt[base:base + kv]
        if clamp and ev_state[v] >= 0:
            w *= float(r[int(ev_state[v])])
            state[v] = int(ev_state[v])
        else:
            state[v] = _pick(u, r)
    return state, w


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_equals_plain_restatement(oracle_mod, case):
    m, ev = case.model, case.ev_state
    topo = kahn_min_order(m)
    ns = min(case.n_samples, case.cpu_samples)
    # likelihood weighting
    got = oracle_mod.lw_run(m, ev, ns, seed=case.seed, s_begin=case.sample_begin, topo=topo, states_cap=ns)
    hist = np.zeros(int(m.k.sum()))
    off = m.node_off
    for i in range(ns):
        st, w = _draw(m, topo, ev, case.seed, case.sample_begin + i, oracle_mod, clamp=True)
        assert got["states"][i].tolist() == st, (i, "states")
        assert got["weights"][i] == w, (i, "weight")
        for v in range(m.n):
            hist[off[v] + st[v]] += w
    if (ev < 0).all():
        assert np.array_equal(got["hist"], hist)
    assert np.allclose(got["hist"], hist, rtol=1e-12, atol=0)
    # rejection sampling: stop at n_accept, and at max_draw
    flags = []
    forward = []
    cap = min(case.max_draw, 2 * ns)
    for i in range(cap):
        st, _ = _draw(m, topo, ev, case.seed, case.sample_begin + i, oracle_mod, clamp=False)
        forward.append(st)
        flags.append(all(st[v] == ev[v] for v in range(m.n) if ev[v] >= 0))
    n_acc = max(1, sum(flags) * 2 // 3)
    for n_accept, max_draw in ((n_acc, cap), (sum(flags) + 3, cap - 1)):
        counts = np.zeros(int(m.k.sum()))
        drawn = accepted = 0
        while accepted < n_accept and drawn < max_draw:
            if flags[drawn]:
                accepted += 1
                for v in range(m.n):
                    counts[off[v] + forward[drawn][v]] += 1.0
            drawn += 1
        c, d, a = oracle_mod.rs_run(m, ev, n_accept, seed=case.seed, max_draw=max_draw, s_begin=case.sample_begin, topo=topo)
        assert (d, a) == (drawn, accepted)
        assert np.array_equal(c, counts)
    case.drop_model()
