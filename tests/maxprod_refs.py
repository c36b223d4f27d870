"""Host references for max-product belief propagation (bn_mpe_*, bayesiannetwork_amd/csrc/bn_maxprod.hpp).  Plain numpy, no GPU.

``run``                   the reference's loop (belief_propagation.hpp:33-158) restated once more, with the fold of pi(v) (:174-200)
                          and of the lambda-messages (:240-266) selectable: mode="sum" is the reference -- pinned bit for bit to
                          oracle.bp_run by tests/test_maxprod_refs.py -- and mode="max" differs in that fold alone.
``brute_max_marginals``   exact enumeration of the joint: every node's max-marginal, the best and the second-best joint probability.

Product orders (as the kernels and oracle/bp_oracle.c): a term of pi(v) is cpt x pi-messages, parents ascending; a term of the
lambda-message to parent jt is (lambda(v)[i] x cpt) x the OTHER parents' pi-messages, ascending.  Sum mode adds front to back from
+0.0 -- pi(v): assignments in table order; lambda-message: own state outer, assignment inner.  Max mode: acc = +0.0, then
acc = x if acc < x else acc over the terms -- a NaN term never replaces acc, so the result is the largest term above +0.0 (else +0.0)
whatever the order.  State of a node: idx = 0, best = b[0]; b[i] > best takes i (lowest index of the largest element; all NaN: 0).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact_refs  # noqa: E402
from bayesiannetwork_amd import Evidence  # noqa: E402

DBL_MIN = np.finfo(np.float64).tiny
DEFAULT_CAP = 10000   # max_sweeps == 0 in mode="max" (bn_maxprod.hpp kMpeDefaultCap)


def _fold(terms, mode):
    """terms [..., T] -> [...]: the fold over the last axis in its order."""
    if mode == "max":
        return np.where(terms > 0, terms, 0.0).max(axis=-1, initial=0.0)
    zero = np.zeros(terms.shape[:-1] + (1,))
    return np.cumsum(np.concatenate([zero, terms], axis=-1), axis=-1)[..., -1]   # (cumsum adds strictly left to right, from +0.0)


def _normalize(vec):
    """belief_propagation.hpp:298-311: left-to-right sum from 0, divide, no zero guard."""
    s = 0.0
    for x in vec:
        s = s + x
    with np.errstate(divide="ignore", invalid="ignore"):
        return vec / s


def decode(vec):
    idx, best = 0, vec[0]
    for i in range(1, len(vec)):
        if vec[i] > best:
            idx, best = i, vec[i]
    return idx


class _Net:
    def __init__(self, model):
        self.m = model
        n = model.n
        self.k = [int(x) for x in model.k]
        self.par = [[int(u) for u in model.parents(v)] for v in range(n)]
        self.node_off = np.concatenate([[0], np.cumsum(model.k)]).astype(np.int64)
        kp = model.k[model.in_idx] if model.n_edges else np.zeros(0, np.int64)
        self.msg_off = np.concatenate([[0], np.cumsum(kp)]).astype(np.int64)
        self.edge0 = [int(model.in_ptr[v]) for v in range(n)]
        self.children = [[] for _ in range(n)]   # (child, CSR edge id), children ascending
        for v in range(n):
            for j, u in enumerate(self.par[v]):
                self.children[u].append((v, self.edge0[v] + j))
        self.cpt = [np.asarray(model.cpt[int(model.cpt_off[v]):int(model.cpt_off[v + 1])], dtype=np.float64)
                    .reshape([self.k[u] for u in self.par[v]] + [self.k[v]]) for v in range(n)]


def _iterate(model, evidence, mode):
    """The loop, one sweep per step: yields (maximum_difference of the sweep, snapshot) where snapshot() gives the beliefs, states and
    messages of the state the sweep left."""
    net = _Net(model)
    n, k = model.n, net.k
    ev = evidence if evidence is not None else Evidence.none()
    # ---- :33-73
    pi = [np.ones(k[v]) for v in range(n)]
    lam = [np.ones(k[v]) for v in range(n)]
    for v in range(n):
        if not net.par[v]:
            pi[v] = net.cpt[v].reshape(-1).copy()
    frozen = [False] * n
    for j in range(ev.ne):
        v = int(ev.node[j])
        frozen[v] = True
        vec = np.asarray(ev.val[int(ev.off[j]):int(ev.off[j]) + k[v]], dtype=np.float64)
        pi[v], lam[v] = vec.copy(), vec.copy()
    n_edges = int(model.n_edges)
    pim = [np.ones(k[int(model.in_idx[e])]) for e in range(n_edges)]
    lkm = [np.ones(k[int(model.in_idx[e])]) for e in range(n_edges)]
    flat = lambda vs: np.concatenate(vs) if vs else np.zeros(0)   # noqa: E731
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        while True:
            npim, nlkm = [None] * n_edges, [None] * n_edges
            npi, nlam = [None] * n, [None] * n
            for v in range(n):
                m, e0 = len(net.par[v]), net.edge0[v]
                # pi-messages into v (:202-218): pi(p) times the lambda-messages of p's OTHER children, ascending
                for j, p in enumerate(net.par[v]):
                    out = pi[p].copy()
                    for (c, e) in net.children[p]:
                        if c != v:
                            out = out * lkm[e]
                    npim[e0 + j] = _normalize(out)
                # lambda-messages out of v (:240-266)
                base = net.cpt[v] * lam[v]                      # (lambda(v)[i] x cpt) first
                for jt in range(m):
                    w = base
                    for j in range(m):
                        if j != jt:
                            shape = [1] * (m + 1)
                            shape[j] = -1
                            w = w * pim[e0 + j].reshape(shape)
                    # element d: own state outer, the other parents' assignment inner (first parent slowest)
                    w = np.moveaxis(np.moveaxis(w, jt, 0), -1, 1).reshape(k[net.par[v][jt]], -1)
                    nlkm[e0 + jt] = _normalize(_fold(w, mode))
                # pi(v) (:174-200)
                if frozen[v]:
                    npi[v] = pi[v]
                else:
                    val = net.cpt[v]
                    for j in range(m):
                        shape = [1] * (m + 1)
                        shape[j] = -1
                        val = val * pim[e0 + j].reshape(shape)
                    npi[v] = _normalize(_fold(val.reshape(-1, k[v]).T, mode))   # element i: assignments in table order
                # lambda(v) (:220-238)
                if frozen[v]:
                    nlam[v] = lam[v]
                else:
                    out = np.ones(k[v])
                    for (_, e) in net.children[v]:
                        out = out * lkm[e]
                    nlam[v] = _normalize(out)
            md = DBL_MIN                                         # :105-131, messages only; std::max drops a NaN
            for e in range(n_edges):
                for old, new in ((pim[e], npim[e]), (lkm[e], nlkm[e])):
                    d = np.abs(new - old)
                    d = d[~np.isnan(d)]
                    if d.size and d.max() > md:
                        md = float(d.max())
            pi, lam, pim, lkm = npi, nlam, npim, nlkm

            def snapshot(pi=pi, lam=lam, pim=pim, lkm=lkm):
                with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                    beliefs = [_normalize(pi[v] * lam[v]) for v in range(n)]  # :151-158
                return {"beliefs": flat(beliefs), "states": np.asarray([decode(b) for b in beliefs], dtype=np.int32),
                        "pi_msg": flat(pim), "lambda_msg": flat(lkm)}
            yield md, snapshot


def run_settings(model, evidence, settings, mode="max"):
    """One trajectory, several stopping rules: settings = [(eps, max_sweeps), ...] -> the list of what run() returns for each (a run
    with a larger eps or a smaller cap is a prefix of the others)."""
    assert mode in ("sum", "max")
    caps = [ms if ms > 0 else (DEFAULT_CAP if mode == "max" else 0) for _, ms in settings]
    out, residuals, sweeps = [None] * len(settings), [], 0
    for md, snapshot in _iterate(model, evidence, mode):
        residuals.append(md)
        sweeps += 1
        snap = None
        for q, (eps, _) in enumerate(settings):
            if out[q] is not None:
                continue
            converged = md < eps                                 # :147 strict <
            if converged or (caps[q] > 0 and sweeps >= caps[q]):
                snap = snap if snap is not None else snapshot()
                out[q] = dict(snap, sweeps=sweeps, residuals=np.asarray(residuals), converged=converged)
        if all(o is not None for o in out):
            return out


def run(model, evidence=None, eps=0.001, max_sweeps=0, mode="max"):
    """Returns dict(beliefs [sum k], states int32 [n], sweeps, residuals [sweeps], pi_msg, lambda_msg, converged).
    mode="sum": max_sweeps == 0 is unbounded like the reference; mode="max": a cap of DEFAULT_CAP sweeps."""
    return run_settings(model, evidence, [(eps, max_sweeps)], mode)[0]


def joint_tensor(model, ev_state=None):
    """The joint P(x, e) over the FREE nodes as a tensor (axes: free nodes ascending), hard evidence ev_state (int [n], -1 free)
    sliced in.  Tiny networks only."""
    n = model.n
    ev_state = np.full(n, -1, dtype=np.int64) if ev_state is None else np.asarray(ev_state, dtype=np.int64)
    free = [v for v in range(n) if ev_state[v] < 0]
    axis_of = {v: a for a, v in enumerate(free)}
    size = int(np.prod([int(model.k[v]) for v in free], dtype=np.int64)) if free else 1
    assert size <= 1 << 22, "joint too large to enumerate"
    joint = np.ones([int(model.k[v]) for v in free])
    for v in range(n):
        ps = [int(u) for u in model.parents(v)]
        t = np.asarray(model.cpt[int(model.cpt_off[v]):int(model.cpt_off[v + 1])]).reshape([int(model.k[u]) for u in ps] + [int(model.k[v])])
        vars_ = ps + [v]
        idx = tuple(int(ev_state[u]) if ev_state[u] >= 0 else slice(None) for u in vars_)
        t = t[idx]
        kept = [u for u in vars_ if ev_state[u] < 0]
        shape = [1] * len(free)
        order = sorted(range(len(kept)), key=lambda a: axis_of[kept[a]])
        t = np.transpose(t, order) if kept else t
        for u in kept:
            shape[axis_of[u]] = int(model.k[u])
        joint = joint * np.reshape(t, shape)
    return joint, free


def brute_max_marginals(model, ev_state=None):
    """(max-marginals node-major [sum k], each node's vector normalised; argmax assignment int32 [n]; best joint probability;
    second-best joint probability).  The max-marginal of node v at state s: the largest joint probability of a complete
    assignment with x_v = s that agrees with the evidence (0 where s contradicts it)."""
    n = model.n
    ev_state = np.full(n, -1, dtype=np.int64) if ev_state is None else np.asarray(ev_state, dtype=np.int64)
    joint, free = joint_tensor(model, ev_state)
    # pinned to exact_refs: summing the other axes out gives exact_joint
    want = exact_refs.exact_joint(model, ev_state)
    off = np.concatenate([[0], np.cumsum(model.k)]).astype(np.int64)
    out = np.zeros(int(off[-1]))
    for a, v in enumerate(free):
        other = tuple(b for b in range(len(free)) if b != a)
        mm = joint.max(axis=other) if other else joint
        sm = joint.sum(axis=other) if other else joint
        assert np.allclose(sm, want[off[v]:off[v + 1]], rtol=1e-10, atol=1e-300)
        out[off[v]:off[v + 1]] = mm / mm.sum()
    flat = joint.reshape(-1)
    best_at = int(np.argmax(flat))
    best = float(flat[best_at])
    second = float(np.partition(flat, -2)[-2]) if flat.size > 1 else 0.0
    states = np.asarray(ev_state, dtype=np.int32).copy()
    if free:
        for v, s in zip(free, np.unravel_index(best_at, joint.shape)):
            states[v] = int(s)
    for v in range(n):
        if ev_state[v] >= 0:
            out[off[v] + int(ev_state[v])] = 1.0
    return out, states, best, second


# ---- the polytree cases of tests/test_maxprod_refs.py and tests/test_maxprod_gpu.py: (n, seed, number of hard-evidence nodes).
# Chosen on the CPU (scripts in the pull request's history: every polytree(n, seed) x 0..3 evidence nodes was enumerated, kept where
# the second-best joint lies below the best by more than a relative 1e-9, the evidence has non-zero probability and the joint has at
# most 2^20 entries).  A case that fails the margin is a test FAILURE, never a skip.
POLYTREE_CASES = [(8, 1, 0), (9, 2, 1), (10, 3, 2), (11, 4, 3), (12, 5, 1), (10, 6, 0), (12, 7, 2), (8, 8, 3)]


def polytree_case(n, seed, n_ev):
    model = exact_refs.polytree(n, arities=(2, 3, 4), max_parents=3, seed=seed, name=f"polytree{n}_s{seed}")
    ev = exact_refs.draw_evidence(model, n_ev, seed=100 + seed) if n_ev else None
    ev_state = ev.hard_states(model) if ev is not None else np.full(model.n, -1, dtype=np.int32)
    return model, ev, ev_state
