"""Plain numpy restatement of Gibbs sampling as include/bn_mi355x.h states it (bn_gibbs_run), vectorised over the chains: the
Philox4x32-10 block of the uniform, the greedy colouring of the moral graph, the start through the oracle's likelihood-weighting
draw (oracle_lw_run in the sampler's visiting order), the sequential scan in (colour, node index) order, one update, the keep rule.
Every operation of the arithmetic is spelled out -- fp64, one multiply per child, sums left to right -- with index arithmetic of its
own (parent lists, no slot tables); the planner's tables are checked by tests/cpp/test_gibbs_plan.cpp.  The GPU tests compare
counts, states, stuck and kept with this exactly; the statistics of the method are checked on it alone (tests/test_gibbs_refs.py)."""
from __future__ import annotations

import numpy as np

from sampler_cases import kahn_min_order

KEY_TAG = 0x47494253
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """One Philox4x32-10 block (Random123).  ctr: four uint32 values or arrays of them, key: two; returns four uint64 arrays that
    hold 32-bit words."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & _LOW for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2            # 32 x 32 -> 64 bits: no overflow
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LOW, n2, p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniform(seed, chains, g, v):
    """u(seed, chain, sweep g, node v) for an array of 64-bit chain ids."""
    chains = np.asarray(chains, dtype=np.uint64)
    zero = np.zeros_like(chains)
    o0, o1, _, _ = philox4x32_10((zero + np.uint64(v), zero + np.uint64(g & 0xFFFFFFFF), chains & _LOW, chains >> _S32),
                                 (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ KEY_TAG))
    U = (o0 << np.uint64(21)) | (o1 >> np.uint64(11))
    return U.astype(np.float64) * (1.0 / 9007199254740992.0)    # (U < 2^53: the conversion is exact)


def children_of(model):
    kids = [[] for _ in range(model.n)]
    for v in range(model.n):
        for p in model.parents(v):
            kids[int(p)].append(v)
    return kids     # ascending: v runs upwards


def moral_neighbours(model):
    nb = [set() for _ in range(model.n)]
    for v in range(model.n):
        fam = [int(p) for p in model.parents(v)] + [v]
        for a in fam:
            nb[a].update(b for b in fam if b != a)
    return nb


def colouring(model):
    """Greedy: nodes in ascending index, each takes the smallest colour no moral neighbour holds."""
    nb = moral_neighbours(model)
    col = np.full(model.n, -1, dtype=np.int32)
    for v in range(model.n):
        used = {int(col[u]) for u in nb[v] if col[u] >= 0}
        c = 0
        while c in used:
            c += 1
        col[v] = c
    return col


def scan_order(model):
    col = colouring(model)
    return sorted(range(model.n), key=lambda v: (int(col[v]), v))


def start_states(model, ev_state, seed, chain_begin, n_chains, oracle):
    """The states oracle_lw_run draws for sample ids [chain_begin, +n_chains): what bn_lw_run + bn_lw_states hand out."""
    if n_chains == 0:
        return np.zeros((0, model.n), dtype=np.uint8)
    o = oracle.lw_run(model, np.asarray(ev_state, dtype=np.int32), n_chains, seed=seed, s_begin=chain_begin, topo=kahn_min_order(model),
                      states_cap=n_chains)
    return o["states"].copy()


def kept_sweeps(sweep_begin, n_sweeps, burn_in, thin):
    return sum(1 for g in range(sweep_begin, sweep_begin + n_sweeps) if g >= burn_in and (g - burn_in) % thin == 0)


def run(model, ev_state, n_chains, n_sweeps, seed, burn_in=0, thin=1, chain_begin=0, sweep_begin=0, init_states=None, oracle=None):
    """bn_gibbs_run.  Returns dict(counts uint64 [sum k], states uint8 [n_chains][n], stuck, kept)."""
    n = model.n
    k = [int(x) for x in model.k]
    ev_state = np.asarray(ev_state, dtype=np.int64)
    parents = [[int(p) for p in model.parents(v)] for v in range(n)]
    kids = children_of(model)
    cpt = np.asarray(model.cpt, dtype=np.float64)
    off = [int(x) for x in model.cpt_off]
    noff = [int(x) for x in model.node_off]
    if init_states is None:
        st = start_states(model, ev_state, seed, chain_begin, n_chains, oracle).astype(np.int64)
    else:
        st = np.array(init_states, dtype=np.int64).reshape(n_chains, n)
        for v in range(n):
            if ev_state[v] >= 0:
                st[:, v] = ev_state[v]
        assert all((st[:, v] < k[v]).all() for v in range(n)), "a start state is not below its node's arity (BN_ERR_ARG)"
    chains = np.uint64(chain_begin) + np.arange(n_chains, dtype=np.uint64)
    order = [v for v in scan_order(model) if ev_state[v] < 0]
    counts = np.zeros(noff[n], dtype=np.uint64)
    stuck = 0
    with np.errstate(all="ignore"):
        for g in range(sweep_begin, sweep_begin + n_sweeps):
            for v in order:
                row = np.zeros(n_chains, dtype=np.int64)
                for p in parents[v]:
                    row = row * k[p] + st[:, p]
                w = []
                for x in range(k[v]):
                    wx = cpt[off[v] + row * k[v] + x]
                    for c in kids[v]:                      # ascending child index, one multiply each
                        rc = np.zeros(n_chains, dtype=np.int64)
                        for p in parents[c]:
                            rc = rc * k[p] + (x if p == v else st[:, p])
                        wx = wx * cpt[off[c] + rc * k[c] + st[:, c]]
                    w.append(wx)
                T = np.zeros(n_chains, dtype=np.float64)
                for x in range(k[v]):
                    T = T + w[x]
                ok = np.isfinite(T) & (T > 0.0)
                stuck += int(n_chains - np.count_nonzero(ok))
                t = uniform(seed, chains, g, v) * T
                run_sum = np.zeros(n_chains, dtype=np.float64)
                pick = np.full(n_chains, -1, dtype=np.int64)
                last = np.full(n_chains, -1, dtype=np.int64)
                for x in range(k[v]):
                    run_sum = run_sum + w[x]
                    last = np.where(w[x] > 0.0, x, last)
                    pick = np.where((pick < 0) & (t < run_sum), x, pick)
                new = np.where(pick >= 0, pick, last)
                st[:, v] = np.where(ok & (new >= 0), new, st[:, v])
            if g >= burn_in and (g - burn_in) % thin == 0:
                for v in range(n):
                    counts[noff[v]:noff[v + 1]] += np.bincount(st[:, v], minlength=k[v]).astype(np.uint64)
    return {"counts": counts, "states": st.astype(np.uint8), "stuck": stuck,
            "kept": kept_sweeps(sweep_begin, n_sweeps, burn_in, thin) * n_chains}


def frequencies(model, states):
    """Node-major state frequencies [sum k] over the rows of `states`."""
    out = []
    for v in range(model.n):
        out.append(np.bincount(states[:, v].astype(np.int64), minlength=int(model.k[v])) / float(states.shape[0]))
    return np.concatenate(out)
