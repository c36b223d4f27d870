"""Plain numpy fp64 restatement of exact MPE on the junction tree as include/bn_mi355x.h states it (bn_jt_mpe_run), built on the
sum restatement tests/jtree_refs.py: the same plan, base potentials and evidence products, every sum replaced by the max fold
(np.max over numpy axes -- the fold has no order), and the decode by backtracking in explicit loops.  The GPU tests compare states,
max-marginals and scale arrays with this bit for bit.  Also: the enumeration of joint x likelihood vectors for soft evidence, the
small cases with their seeds, the tie networks, and the checks for networks too large to enumerate."""
from __future__ import annotations

import itertools

import numpy as np

from bayesiannetwork_amd import Evidence, FlatModel, from_parent_lists, synth

import exact_refs as xr
import jtree_refs as jr
import maxprod_refs as mr


def _max_fold(m):
    """m [S, T]: per row the max fold of its T terms -- the largest term above +0.0, else +0.0; a NaN never wins."""
    return np.max(np.where(m > 0, m, 0.0), axis=1, initial=0.0)


def _onto_max(arr, big, sub, k):
    """The max folds of table `arr` over `big` onto `sub`."""
    first = [i for i, u in enumerate(big) if u in sub]
    rest = [i for i, u in enumerate(big) if u not in sub]
    s = int(np.prod([k[big[i]] for i in first], dtype=np.int64)) if first else 1
    return _max_fold(np.transpose(arr, first + rest).reshape(s, -1))


class Restatement(jr.Restatement):
    """``run_max(evidence)`` -> (states int32 [n], max-marginals [sum k], scales [cliques], log max_x P(x, e))."""

    def _pick(self, tab, c, fixed):
        """The lowest entry index of the largest entry of clique c's table among the entries that agree with `fixed` (variable ->
        state): the entries in ascending entry index (first variable most significant), best = t[0], t[i] > best takes i."""
        k, cl = self.k, self.cl[c]
        ranges = [[fixed[u]] if u in fixed else range(k[u]) for u in cl]
        best, at = None, None
        for digits in itertools.product(*ranges):   # ascending entry index
            x = tab[digits]
            if best is None or x > best:
                best, at = x, digits
        return at

    def run_max(self, evidence=None):
        k, cl, sp, par = self.k, self.cl, self.sp, self.par
        nc = len(cl)
        ev = {}
        if evidence is not None:
            for j in range(evidence.ne):
                ev[int(evidence.node[j])] = np.asarray(evidence.val[evidence.off[j]:evidence.off[j + 1]], dtype=np.float64)
        pot = []
        for c in range(nc):
            arr = self.psi0[c]
            for v in self.homed[c]:
                if v in ev:
                    arr = arr * jr._spread(ev[v], {v}, cl[c], k)
            pot.append(arr)
        scales = np.zeros(nc)
        msg = [None] * nc
        with np.errstate(all="ignore"):
            for l in range(len(self.by_level) - 1, -1, -1):
                for c in self.by_level[l]:
                    raw = _onto_max(pot[c], cl[c], set(sp[c]), k)
                    s = float(_max_fold(raw.reshape(1, -1))[0])
                    scales[c] = s
                    msg[c] = raw / s if s > 0 else raw
                if l == 0:
                    break
                for p in self.by_level[l - 1]:
                    for c in self.kids[p]:   # ascending child id
                        pot[p] = pot[p] * jr._spread(msg[c], set(sp[c]), cl[p], k)
            collected = list(pot)   # (the products above made new arrays: these stay as collect left them)
            for l in range(1, len(self.by_level)):
                for c in self.by_level[l]:
                    new = _onto_max(pot[par[c]], cl[par[c]], set(sp[c]), k)
                    ratio = np.where(msg[c] == 0.0, 0.0, new / msg[c])
                    pot[c] = pot[c] * jr._spread(ratio, set(sp[c]), cl[c], k)
            out = []
            for v in range(self.model.n):
                h = int(self.plan["home"][v])
                u = _onto_max(pot[h], cl[h], {v}, k)
                out.append(u / jr._left_to_right(u))
            lg = 0.0
            for s in scales:
                lg = lg + float(np.log(s))
        # decode: top down, every clique from its entries after collect
        pick = [None] * nc
        for l in range(len(self.by_level)):
            for c in self.by_level[l]:
                fixed = {}
                if par[c] >= 0:
                    up = dict(zip(cl[par[c]], pick[par[c]]))
                    fixed = {u: up[u] for u in sp[c]}
                pick[c] = self._pick(collected[c], c, fixed)
        states = np.zeros(self.model.n, dtype=np.int32)
        for v in range(self.model.n):
            h = int(self.plan["home"][v])
            states[v] = pick[h][cl[h].index(v)]
        return states, np.concatenate(out), scales, lg


# ---- enumeration ---------------------------------------------------------------------------------------------------------------

def enumerate_mpe(model, evidence=None):
    """(max-marginals node-major [sum k], each vector normalised; argmax assignment int32 [n]; best; second best) of
    P(x) x the likelihood vectors of `evidence`, hard or soft, over ALL nodes.  Tiny networks only."""
    joint, free = mr.joint_tensor(model)
    assert free == list(range(model.n))
    if evidence is not None:
        for j in range(evidence.ne):
            v = int(evidence.node[j])
            shape = [1] * model.n
            shape[v] = -1
            joint = joint * np.asarray(evidence.val[evidence.off[j]:evidence.off[j + 1]], dtype=np.float64).reshape(shape)
    out = []
    for v in range(model.n):
        mm = joint.max(axis=tuple(b for b in range(model.n) if b != v)) if model.n > 1 else joint
        with np.errstate(invalid="ignore"):
            out.append(mm / mm.sum())
    flat = joint.reshape(-1)
    at = int(np.argmax(flat))
    second = float(np.partition(flat, -2)[-2]) if flat.size > 1 else 0.0
    return np.concatenate(out), np.asarray(np.unravel_index(at, joint.shape), dtype=np.int32), float(flat[at]), second


# ---- the small cases: name -> model.  The seeds were chosen on the CPU: for every case and each of its three evidence kinds (none,
# two hard nodes, one soft vector: small_evidence) the second-best joint lies below the best by more than a relative 1e-9, and the
# evidence has non-zero probability.  A case that fails the margin is a test FAILURE, never a skip.
SMALL_SEEDS = {"grid3x3k3": 1, "grid2x5k4": 1, "dag10": 3}


def small_cases():
    out = {"pearl": synth.pearl(), "grid3x3k3": synth.grid(3, 3, 3, seed=SMALL_SEEDS["grid3x3k3"]),
           "grid2x5k4": synth.grid(2, 5, 4, seed=SMALL_SEEDS["grid2x5k4"]),
           "dag10": synth.random_dag(10, 3, 8, [2, 3, 4], seed=SMALL_SEEDS["dag10"])}
    for n, seed, n_ev in mr.POLYTREE_CASES:
        out[f"polytree{n}_s{seed}"] = mr.polytree_case(n, seed, n_ev)[0]
    return out


def small_evidence(model):
    """[(kind, evidence)]: none; two hard nodes at the states of one forward sample; one strictly positive soft vector."""
    rng = np.random.default_rng(1000 + model.n)
    v = model.n // 2
    return [("none", None), ("hard2", xr.draw_evidence(model, 2, seed=11)),
            ("soft", Evidence.from_dict(model, {v: 0.1 + rng.random(int(model.k[v]))}))]


def tie_pair():
    """Node 0 uniform over two states, node 1 = "not node 0": 0.5 on (0, 1) and on (1, 0), both max-marginals [0.5, 0.5]."""
    return from_parent_lists([2, 2], [[], [0]], [np.asarray([0.5, 0.5]), np.asarray([0.0, 1.0, 1.0, 0.0])], name="tie_pair")


def tie_grid():
    """grid(3, 3, 2) with every CPT entry 0.5: all 512 assignments tie."""
    g = synth.grid(3, 3, 2, seed=1)
    return FlatModel(g.k, g.in_ptr, g.in_idx, g.cpt_off, np.full(g.cpt.shape, 0.5), name="tie_grid")


# ---- the decode's two special paths: roots only (one level: the states pay a barrier of their own), and a childless root beside
# deeper cliques.  name -> model.  Every case passes the margin of the small cases with both kinds of forest_evidence.
def forest_cases():
    a = np.asarray
    return {"lone": from_parent_lists([3], [[]], [a([0.2, 0.5, 0.3])], name="lone"),                                   # 1 clique, 1 level
            "two": from_parent_lists([2, 3], [[], []], [a([0.25, 0.75]), a([0.2, 0.5, 0.3])], name="two"),             # 2 roots, 1 level
            "forest": from_parent_lists([3, 2, 2, 2], [[], [], [1], [2]],                                              # levels [0, 0, 1]
                                        [a([0.2, 0.5, 0.3]), a([0.25, 0.75]), a([0.9, 0.1, 0.3, 0.7]), a([0.6, 0.4, 0.2, 0.8])], name="forest")}


def forest_evidence(model):
    """[(kind, evidence)]: none; one strictly positive soft vector on node n // 2."""
    v = model.n // 2
    return [("none", None), ("soft", Evidence.from_dict(model, {v: 0.1 + np.random.default_rng(7).random(int(model.k[v]))}))]


# ---- networks too large to enumerate -------------------------------------------------------------------------------------------

def _log_terms(model, states, ev):
    """Per node: log cpt_v[x] (+ log of v's evidence value at x_v)."""
    out = np.zeros(model.n)
    with np.errstate(divide="ignore"):
        for v in range(model.n):
            out[v] = _node_term(model, states, ev, v)
    return out


def _node_term(model, states, ev, v):
    row = 0
    for u in model.parents(v):
        row = row * int(model.k[u]) + int(states[u])
    with np.errstate(divide="ignore"):
        t = float(np.log(model.cpt[int(model.cpt_off[v]) + row * int(model.k[v]) + int(states[v])]))
        if v in ev:
            t += float(np.log(ev[v][int(states[v])]))
    return t


def check_large(model, evidence, states, max_marginals, log_p):
    """The checks of a decoded assignment on a network that cannot be enumerated: it agrees with the (hard) evidence; its log
    probability is the claimed maximum; no single-node flip raises it; a node's state is the argmax of its max-marginal wherever
    the vector's top two entries differ by more than a relative 1e-9."""
    ev = {}
    if evidence is not None:
        for j in range(evidence.ne):
            ev[int(evidence.node[j])] = np.asarray(evidence.val[evidence.off[j]:evidence.off[j + 1]], dtype=np.float64)
    for v, vec in ev.items():
        assert vec[int(states[v])] > 0, ("the state of an evidence node contradicts it", v)
    terms = _log_terms(model, states, ev)
    total = 0.0
    for t in terms:
        total += float(t)
    assert np.isfinite(total) and abs(total - log_p) <= 1e-12 * float(np.abs(terms).sum()), (total, log_p)
    children = [[] for _ in range(model.n)]
    for v in range(model.n):
        for u in model.parents(v):
            children[int(u)].append(v)
    x = np.asarray(states, dtype=np.int64).copy()
    for v in range(model.n):
        local = [v] + children[v]
        old = [float(terms[u]) for u in local]
        for s in range(int(model.k[v])):
            if s == states[v]:
                continue
            x[v] = s
            new = [_node_term(model, x, ev, u) for u in local]
            # (a sum of a handful of logarithms: its rounding is far below 1e-12 of the terms' magnitudes)
            assert sum(new) - sum(old) <= 1e-12 * (sum(abs(t) for t in old) + sum(abs(t) for t in new if np.isfinite(t))), ("a flip raises the probability", v, s)
        x[v] = states[v]
    off = model.node_off
    for v in range(model.n):
        vec = np.asarray(max_marginals[off[v]:off[v + 1]])
        top = np.sort(vec)[::-1]
        if vec.size == 1 or top[0] - top[1] > 1e-9 * top[0]:
            assert int(np.argmax(vec)) == int(states[v]), ("state is not the argmax of a decided max-marginal", v)
