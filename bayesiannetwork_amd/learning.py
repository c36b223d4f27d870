"""Mirror of bn::learning (reference bayesian/learning/greedy.hpp, k2_algorithm.hpp, brute_force.hpp, stepwise_structure.hpp):
structure search under AIC / MDL on the GPU (bn_learn_* of include/bn_mi355x.h).

AIC and MDL are decomposable, so a candidate edge u -> c changes the family term of c and the parameter count and nothing else.
`score_groups` scores many candidate families of a child in one pass over an `InfoTable`; `Learner` holds a graph, its family
terms and its score, and `Learner.try_parents` is the reference's inner loop for one child; `Greedy` and `K2` are the reference's
functors on top of it.  `score_subsets` scores EVERY subset of a candidate parent set of one child from one pass over the table
(the subset lattice); `Learner.best_parents`, `BruteForce` and `StepwiseStructure` are the exhaustive searches on top of that.
The learner's score takes the DEVICE's fp64 logarithm (the header states the function); `AIC` / `MDL` of
the learned model through evaluation.py agree with it to a few ulp per term, not bit for bit.

Differences from the reference: a family is limited to 16 parents (`max_parents` may lower that) and 2^20 table entries -- a
candidate beyond them is not added; the returned model carries CPTs fitted to the FINAL structure (the reference leaves the CPTs of
the last rejected candidate in the graph); `seed=` / `orders=` make the shuffles reproducible."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from .evaluation import AIC, MDL, InfoTable, table_from_sampler
from .flat import FlatModel

MAX_PARENTS = 16


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _criterion(c) -> int:
    if isinstance(c, str) and c.lower() in ("aic", "mdl"):
        return 0 if c.lower() == "aic" else 1
    if c is AIC or isinstance(c, AIC):
        return 0
    if c is MDL or isinstance(c, MDL):
        return 1
    raise ValueError('criterion: "aic", "mdl", or the AIC / MDL classes')


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    for i, x in enumerate(lists):
        ptr[i + 1] = ptr[i] + len(x)
    idx = np.array([int(v) for x in lists for v in x], dtype=np.int32)
    return ptr, idx


def score_groups(table: InfoTable, groups, counts: bool = False, splits: int = 0):
    """groups: [(child, base parents (strictly increasing), candidates), ...].  Returns per group the list of family terms
    [ll(base), ll(base + u_0), ...]; counts=True: (that, per group the list of uint64 count arrays in the fitted layout).
    splits > 0 fixes the number of workgroups the patterns are split over (no result depends on it)."""
    groups = [(int(c), [int(x) for x in b], [int(x) for x in u]) for c, b, u in groups]
    child = np.array([g[0] for g in groups], dtype=np.int32)
    bptr, bidx = _csr([g[1] for g in groups])
    cptr, cidx = _csr([g[2] for g in groups])
    n_fam = len(groups) + len(cidx)
    ll = np.zeros(max(n_fam, 1))
    N = None
    sizes = []
    if counts:
        k = table.k
        for c, b, u in groups:
            if not (0 <= c < table.n and all(0 <= x < table.n for x in b + u)):
                sizes = None   # (out of range: the library names the group)
                break
            base = int(k[c])
            for x in b:
                base *= int(k[x])
            sizes.append([base] + [base * int(k[x]) for x in u])
        N = np.zeros(max(sum(map(sum, sizes)) if sizes else 1, 1), dtype=np.uint64)
        if sizes is not None and N.size > (1 << 28):
            raise ValueError("the counts of this batch need more than 2 GiB")
    old = os.environ.get("BN_LEARN_SPLITS")
    if splits > 0:
        os.environ["BN_LEARN_SPLITS"] = str(int(splits))
    try:
        _lib.check(_lib.lib().bn_learn_score_groups(table._h, len(groups), _p(child, ctypes.c_int32), _p(bptr, ctypes.c_int32),
                                                    _p(bidx, ctypes.c_int32), _p(cptr, ctypes.c_int32), _p(cidx, ctypes.c_int32),
                                                    _p(ll, ctypes.c_double), _p(N, ctypes.c_uint64) if counts else None))
    finally:
        if splits > 0:
            if old is None:
                del os.environ["BN_LEARN_SPLITS"]
            else:
                os.environ["BN_LEARN_SPLITS"] = old
    out, at = [], 0
    for c, b, u in groups:
        out.append(ll[at:at + 1 + len(u)].tolist())
        at += 1 + len(u)
    if not counts:
        return out
    blocks, at = [], 0
    for s in sizes:
        row = []
        for x in s:
            row.append(N[at:at + x])
            at += x
        blocks.append(row)
    return out, blocks


def score_subsets(table: InfoTable, child: int, base, cand, counts: bool = False, splits: int = 0):
    """The family terms of `child` with the parents base + S for every subset S of `cand`: a list of 2^m values, entry `mask`
    standing for S = {cand[j] : bit j of mask}.  counts=True: (that, the list of the 2^m uint64 count arrays in the fitted
    layout).  One count of the top family base + cand; every other family is summed out of it on the device."""
    base = np.ascontiguousarray([int(x) for x in base], dtype=np.int32)
    cand = np.ascontiguousarray([int(x) for x in cand], dtype=np.int32)
    m = len(cand)
    if m > MAX_PARENTS:
        raise ValueError(f"{m} candidates: at most {MAX_PARENTS} minus the base parents")
    ll = np.zeros(1 << m)
    N, sizes = None, None
    if counts:
        k = table.k
        if 0 <= int(child) < table.n and all(0 <= int(x) < table.n for x in list(base) + list(cand)):
            cells = int(k[int(child)]) * int(np.prod([int(k[x]) for x in base], dtype=np.int64))
            sizes = [cells * int(np.prod([int(k[cand[j]]) for j in range(m) if (mask >> j) & 1], dtype=np.int64)) for mask in range(1 << m)]
        total = sum(sizes) if sizes else 1
        if total > (1 << 25):
            sizes, total = None, 1   # (over the limit: the library says so)
        N = np.zeros(max(total, 1), dtype=np.uint64)
    old = os.environ.get("BN_LEARN_SPLITS")
    if splits > 0:
        os.environ["BN_LEARN_SPLITS"] = str(int(splits))
    try:
        _lib.check(_lib.lib().bn_learn_score_subsets(table._h, int(child), len(base), _p(base, ctypes.c_int32), m, _p(cand, ctypes.c_int32),
                                                     _p(ll, ctypes.c_double), _p(N, ctypes.c_uint64) if counts else None))
    finally:
        if splits > 0:
            if old is None:
                del os.environ["BN_LEARN_SPLITS"]
            else:
                os.environ["BN_LEARN_SPLITS"] = old
    if not counts:
        return ll.tolist()
    blocks, at = [], 0
    for x in sizes:
        blocks.append(N[at:at + x])
        at += x
    return ll.tolist(), blocks


class Learner:
    """bn_learner: a graph over the columns of `table`, its family terms and its score.  `structure`: None (no edges), a
    FlatModel, or per-node parent lists."""

    def __init__(self, table: InfoTable, structure=None, criterion="aic", max_parents: int = MAX_PARENTS):
        if structure is None:
            parents = [[] for _ in range(table.n)]
        elif isinstance(structure, FlatModel):
            parents = [structure.parents(v).tolist() for v in range(structure.n)]
        else:
            parents = [list(p) for p in structure]
        if len(parents) != table.n:
            raise ValueError(f"the structure has {len(parents)} nodes, the table {table.n} columns")
        ptr, idx = _csr(parents)
        self.table, self.n = table, table.n
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().bn_learn_create(table._h, _p(ptr, ctypes.c_int32), _p(idx, ctypes.c_int32), _criterion(criterion),
                                              int(max_parents), ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().bn_learn_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def try_parents(self, child: int, candidates) -> np.ndarray:
        """The reference's inner loop for `child` over `candidates` in the given order; bool per candidate: edge added."""
        cand = np.ascontiguousarray(candidates, dtype=np.int32).reshape(-1)
        acc = np.zeros(max(len(cand), 1), dtype=np.uint8)
        _lib.check(_lib.lib().bn_learn_try_parents(self._h, int(child), len(cand), _p(cand, ctypes.c_int32), _p(acc, ctypes.c_uint8)))
        return acc[:len(cand)].astype(bool)

    def best_parents(self, child: int, candidates) -> np.ndarray:
        """Adds the best subset of `candidates` to the parents of `child` (every subset scored through the subset lattice; the
        strictly smallest score, among equals the first in the reference's visiting order); bool per candidate: edge added."""
        cand = np.ascontiguousarray(candidates, dtype=np.int32).reshape(-1)
        taken = np.zeros(max(len(cand), 1), dtype=np.uint8)
        _lib.check(_lib.lib().bn_learn_best_parents(self._h, int(child), len(cand), _p(cand, ctypes.c_int32), _p(taken, ctypes.c_uint8)))
        return taken[:len(cand)].astype(bool)

    def terms(self):
        """(ll [n], parameters): the family terms and the parameter count the score is made of."""
        ll = np.zeros(max(self.n, 1))
        params = ctypes.c_int64()
        _lib.check(_lib.lib().bn_learn_terms(self._h, _p(ll, ctypes.c_double), ctypes.byref(params)))
        return ll[:self.n], params.value

    def brute_force(self, vertexes) -> float:
        """brute_force::operator()(graph, vertexes) on this learner's graph (at most 8 vertexes); returns the reference's
        evaluated quantity: the likelihood over `vertexes` in the given order plus the penalty of the whole graph."""
        vs = np.ascontiguousarray(vertexes, dtype=np.int32).reshape(-1)
        out = ctypes.c_double()
        _lib.check(_lib.lib().bn_learn_brute_force(self._h, len(vs), _p(vs, ctypes.c_int32), ctypes.byref(out)))
        return out.value

    def brute_force_hint(self, parent_nodes, child_nodes) -> float:
        """brute_force::learn_with_hint on this learner's graph; returns the score."""
        ps = np.ascontiguousarray(parent_nodes, dtype=np.int32).reshape(-1)
        cs = np.ascontiguousarray(child_nodes, dtype=np.int32).reshape(-1)
        _lib.check(_lib.lib().bn_learn_brute_force_hint(self._h, len(ps), _p(ps, ctypes.c_int32), len(cs), _p(cs, ctypes.c_int32)))
        return self.score()

    def score(self) -> float:
        out = ctypes.c_double()
        _lib.check(_lib.lib().bn_learn_score(self._h, ctypes.byref(out)))
        return out.value

    def info(self, name: str) -> int:
        out = ctypes.c_int64()
        _lib.check(_lib.lib().bn_learn_get(self._h, name.encode(), ctypes.byref(out)))
        return out.value

    def structure(self):
        """(in_ptr [n + 1], in_idx [edges]), parents increasing per node."""
        ptr = np.zeros(self.n + 1, dtype=np.int32)
        idx = np.zeros(max(self.info("edges"), 1), dtype=np.int32)
        _lib.check(_lib.lib().bn_learn_structure(self._h, _p(ptr, ctypes.c_int32), _p(idx, ctypes.c_int32)))
        return ptr, idx[:int(ptr[-1])].copy()

    def parents(self):
        ptr, idx = self.structure()
        return [idx[ptr[v]:ptr[v + 1]].tolist() for v in range(self.n)]


def structure_model(k, in_ptr, in_idx, name: str = "") -> FlatModel:
    """A FlatModel of the given structure with an all-zero CPT of the right size."""
    k = np.asarray(k, dtype=np.int32)
    sizes = k.astype(np.int64).copy()
    for v in range(len(k)):
        for u in in_idx[in_ptr[v]:in_ptr[v + 1]]:
            sizes[v] *= int(k[u])
    cpt_off = np.zeros(len(k) + 1, dtype=np.int64)
    np.cumsum(sizes, out=cpt_off[1:])
    return FlatModel(k, in_ptr, in_idx, cpt_off, np.zeros(int(cpt_off[-1])), name=name)


class _Search:
    def __init__(self, criterion, sampling, max_parents: int = MAX_PARENTS, seed=None, device: int = _lib.BN_DEVICE_CURRENT):
        self._criterion, self._sampling, self._max_parents, self._device = _criterion(criterion), sampling, int(max_parents), device
        self._rng = np.random.default_rng(seed)
        self._table = sampling if isinstance(sampling, InfoTable) else None
        self.last = {}   # counters of the last search: families_scored, passes, count_ns, score_ns, lattice_ns, subsets_scored

    def _ensure_table(self, model) -> InfoTable:
        if self._table is None:
            self._table = table_from_sampler(self._sampling, range(model.n), model.k, self._device)
        return self._table

    def _learner(self, model) -> Learner:
        return Learner(self._ensure_table(model), model, "aic" if self._criterion == 0 else "mdl", self._max_parents)

    def _finish(self, model, L: Learner):
        from .engine import fit_cpt
        ptr, idx = L.structure()
        out = structure_model(model.k, ptr, idx, name=model.name)
        t = self._table
        out.cpt[:] = fit_cpt(out, t.patterns, t.counts, device=t.device)
        self.last = {name: L.info(name) for name in ("families_scored", "passes", "count_ns", "score_ns", "lattice_ns", "subsets_scored")}
        return out, L.score()


class Greedy(_Search):
    """bn::learning::greedy<Eval> (greedy.hpp).  `greedy(model)`, `greedy(model, vertexes)`, `greedy.learn_with_hint(model,
    parent_nodes, child_nodes)`; `model` gives the arities and the starting graph (its CPTs are not read).  Each returns
    (learned FlatModel, score).  orders=(children, tails): the order the children are visited in and, per child, the order of
    its candidates, in place of the shuffles.  `run_on` / `hint_on` are the same loops on a given Learner."""

    def run_on(self, L: Learner, vertexes=None, orders=None) -> float:
        if orders is not None:
            for child, tail in zip(*orders):
                L.try_parents(child, tail)
            return L.score()
        vs = [int(v) for v in (range(L.n) if vertexes is None else vertexes)]
        vs = [vs[i] for i in self._rng.permutation(len(vs))]   # (:28)
        for i in range(len(vs)):
            tail = vs[i + 1:]
            vs[i + 1:] = [tail[j] for j in self._rng.permutation(len(tail))]   # (:37: the shuffles of the tail accumulate)
            L.try_parents(vs[i], vs[i + 1:])
        return L.score()

    def hint_on(self, L: Learner, parent_nodes, child_nodes, orders=None) -> float:
        if orders is not None:
            for child, ps in zip(*orders):
                L.try_parents(child, ps)
            return L.score()
        cs = [int(v) for v in child_nodes]
        cs = [cs[i] for i in self._rng.permutation(len(cs))]   # (:70)
        ps = [int(v) for v in parent_nodes]
        for child in cs:
            ps = [ps[i] for i in self._rng.permutation(len(ps))]   # (:80)
            L.try_parents(child, ps)
        return L.score()

    def __call__(self, model, vertexes=None, orders=None):
        if orders is None and vertexes is None:
            vertexes = range(model.n)
        with self._learner(model) as L:
            self.run_on(L, vertexes, orders)
            return self._finish(model, L)

    def learn_with_hint(self, model, parent_nodes, child_nodes, orders=None):
        with self._learner(model) as L:
            self.hint_on(L, parent_nodes, child_nodes, orders)
            return self._finish(model, L)


class K2(_Search):
    """bn::learning::k2_algorithm<Eval> (k2_algorithm.hpp).  `k2(model, precondition)`: precondition {node: [nodes that may not
    become its parents]}; every other node is a candidate, in node order.  orders=children replaces the shuffle of the targets.
    `run_on` is the same loop on a given Learner."""

    def run_on(self, L: Learner, precondition=None, orders=None) -> float:
        pre = {int(v): [int(x) for x in xs] for v, xs in (precondition or {}).items()}
        if orders is None:
            vs = [int(v) for v in self._rng.permutation(L.n)]   # (:30)
        else:
            vs = [int(v) for v in orders]
        for target in vs:
            cand = [v for v in range(L.n) if v != target and v not in pre.get(target, ())]   # (:35-45)
            for u, ok in zip(cand, L.try_parents(target, cand)):
                if ok:
                    pre.setdefault(u, []).append(target)   # (:57)
        return L.score()

    def __call__(self, model, precondition=None, orders=None):
        with self._learner(model) as L:
            self.run_on(L, precondition, orders)
            return self._finish(model, L)


class BruteForce(_Search):
    """bn::learning::brute_force<Eval> (brute_force.hpp).  `bf(model)`, `bf(model, vertexes)`: the reference's enumeration over
    at most 8 vertexes (no edge / one way / the other way per level); `bf.learn_with_hint(model, parent_nodes, child_nodes)`:
    every subset of the edges parent -> child.  Family terms come from the subset lattice, one device call per vertex or child.
    Each returns (FlatModel with CPTs fitted to the final structure, the learner's whole-graph score) like `Greedy`;
    `last_eval` is the reference's return value of the last `bf(model, vertexes)`: the likelihood over `vertexes` only."""

    last_eval = None

    def run_on(self, L: Learner, vertexes=None, orders=None) -> float:
        self.last_eval = L.brute_force(range(L.n) if vertexes is None else vertexes)
        return L.score()

    def hint_on(self, L: Learner, parent_nodes, child_nodes, orders=None) -> float:
        return L.brute_force_hint(parent_nodes, child_nodes)

    def __call__(self, model, vertexes=None):
        with self._learner(model) as L:
            self.run_on(L, vertexes)
            return self._finish(model, L)

    def learn_with_hint(self, model, parent_nodes, child_nodes):
        with self._learner(model) as L:
            self.hint_on(L, parent_nodes, child_nodes)
            return self._finish(model, L)


class StepwiseStructure(_Search):
    """bn::learning::stepwise_structure<Eval, InnerLearning, BetweenLearning> (stepwise_structure.hpp): the edges are cleared; the
    shuffled nodes are dealt round-robin into ceil(n / initial_cluster_size) clusters; `inner` learns each cluster
    (`inner.run_on(L, cluster)`); then random ordered pairs (parent cluster, child cluster) are merged through
    `between.hint_on(L, parent, child)` until one cluster is left.  Everything runs on ONE Learner, so the table is uploaded once.
    `inner` / `between`: classes with Greedy's constructor (BruteForce, Greedy), or instances.  plan=(clusters, [(parent_index,
    child_index), ...]) replaces the random draws; `last_plan` records what a run did, in that form.  Returns (FlatModel with
    fitted CPTs, the final whole-graph score).  The reference returns DBL_MAX when there was nothing to merge (one cluster from
    the start); here the score is the learner's in that case too."""

    def __init__(self, criterion, sampling, inner=None, between=None, seed=None, max_parents: int = MAX_PARENTS,
                 device: int = _lib.BN_DEVICE_CURRENT):
        super().__init__(criterion, sampling, max_parents, seed, device)
        self._inner = BruteForce if inner is None else inner
        self._between = Greedy if between is None else between
        self._seeded = seed is not None
        self.last_plan = None

    def _make(self, kind):
        if not isinstance(kind, type):
            return kind
        seed = int(self._rng.integers(1 << 32)) if self._seeded else None
        return kind("aic" if self._criterion == 0 else "mdl", self._table, max_parents=self._max_parents, seed=seed, device=self._device)

    def __call__(self, model, initial_cluster_size: int, plan=None):
        size = int(initial_cluster_size)
        if size <= 0:
            raise ValueError("initial_cluster_size must be positive")
        table = self._ensure_table(model)
        inner, between = self._make(self._inner), self._make(self._between)
        with Learner(table, None, "aic" if self._criterion == 0 else "mdl", self._max_parents) as L:   # (:26: erase_all_edge)
            n = L.n
            if plan is not None:
                clusters = [[int(v) for v in c] for c in plan[0]]
                pairs = [(int(p), int(c)) for p, c in plan[1]]
            else:
                cluster_num = n // size + (1 if n % size else 0)   # (:47)
                clusters = [[] for _ in range(cluster_num)]
                for i, v in enumerate(self._rng.permutation(n)):   # (:53-61)
                    clusters[i % cluster_num].append(int(v))
                pairs = None
            done_clusters, done_pairs = [list(c) for c in clusters], []
            for cluster in clusters:   # (:71)
                inner.run_on(L, cluster)
            step = 0
            while len(clusters) != 1:   # (:82)
                if pairs is not None:
                    if step >= len(pairs):
                        raise ValueError("the plan ends before one cluster is left")
                    parent_index, child_index = pairs[step]
                    if parent_index == child_index or not (0 <= parent_index < len(clusters) and 0 <= child_index < len(clusters)):
                        raise ValueError(f"plan step {step}: bad cluster pair {pairs[step]}")
                else:
                    child_index = int(self._rng.integers(len(clusters)))   # (:85-88)
                    parent_index = child_index
                    while parent_index == child_index:
                        parent_index = int(self._rng.integers(len(clusters)))
                step += 1
                done_pairs.append((parent_index, child_index))
                parent, child = clusters[parent_index], clusters[child_index]
                between.hint_on(L, parent, child)   # (:92)
                merged = parent + child
                for i in sorted((parent_index, child_index), reverse=True):   # (:101-103)
                    del clusters[i]
                clusters.append(merged)
            self.last_plan = (done_clusters, done_pairs)
            return self._finish(model, L)
