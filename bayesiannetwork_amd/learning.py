"""Mirror of bn::learning (reference bayesian/learning/greedy.hpp, k2_algorithm.hpp, brute_force.hpp, stepwise_structure.hpp):
structure search under AIC / MDL, BDeu or the K2 score on the GPU (bn_learn_* of include/bn_mi355x.h).  Every class and function
here takes `criterion`: "aic", "mdl", "bdeu", "k2score", or the AIC / MDL / BDeu / K2Score classes or instances (`BDeu(10)` for
another equivalent sample size).  Under BDeu and K2 the score is minus the log marginal likelihood, no penalty: smaller is better.

AIC and MDL are decomposable, so a candidate edge u -> c changes the family term of c and the parameter count and nothing else.
`score_groups` scores many candidate families of a child in one pass over an `InfoTable`; `Learner` holds a graph, its family
terms and its score, and `Learner.try_parents` is the reference's inner loop for one child; `Greedy` and `K2` are the reference's
functors on top of it.  `score_subsets` scores EVERY subset of a candidate parent set of one child from one pass over the table
(the subset lattice); `Learner.best_parents`, `BruteForce` and `StepwiseStructure` are the exhaustive searches on top of that.
`TermTable` holds the family term of every parent set of at most `max_parents` nodes per child on the device; `Learner.anneal` runs
the reference's simulated annealing (simulated_annealing.hpp) as many independent device-resident chains over it, and
`SimulatedAnnealing` is the reference's functor on top of that.  `Learner.hc` runs the reference's hierarchical clustering with
stochastic pruning (stepwise_structure_hc.hpp) as many device-resident runs over the same table and the all-pairs mutual
information; `StepwiseStructureHC` is its functor.  `Learner.climb` is tabu hill climbing over add, delete and reverse moves (not in
the reference) as device-resident runs over the same table; `HillClimbing` is its functor.
`PC` is constraint-based learning (not in the reference): the PC-stable skeleton from G^2 conditional-independence tests decided level
by level on the device (bn_learn_pc), then v-structures and Meek's rules; it returns the equivalence class (`PCResult.cpdag`) with
the separating sets, and `cpdag_to_dag` gives one DAG of the class, which can seed a `Learner`.
The learner's score takes the DEVICE's fp64 logarithm (the header states the function); `AIC` / `MDL` of
the learned model through evaluation.py agree with it to a few ulp per term, not bit for bit.

Differences from the reference: a family is limited to 16 parents (`max_parents` may lower that) and 2^20 table entries -- a
candidate beyond them is not added; the returned model carries CPTs fitted to the FINAL structure (the reference leaves the CPTs of
the last rejected candidate in the graph); `seed=` / `orders=` make the shuffles reproducible.
`ChowLiu` and `TAN` (not in the reference; bnlearn's chow.liu / tree.bayes) are the tree learners: the maximum spanning tree of the
all-pairs (class-conditional) mutual information, both matrices and the tree made on the device (bn_learn_tree); `max_spanning_tree`
is the tree of any weight matrix under the library's edge order."""
from __future__ import annotations

import contextlib
import ctypes
import os

import numpy as np

from . import _lib
from .evaluation import AIC, MDL, BDeu, InfoTable, K2Score, table_from_sampler
from .flat import FlatModel

MAX_PARENTS = 16


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _canon(c):
    """A criterion in the form the classes here pass on: "aic", "mdl", a BDeu instance or a K2Score instance."""
    if isinstance(c, str) and c.lower() in ("aic", "mdl"):
        return c.lower()
    if c is AIC or isinstance(c, AIC):
        return "aic"
    if c is MDL or isinstance(c, MDL):
        return "mdl"
    if isinstance(c, (BDeu, K2Score)):
        return c
    if c is BDeu or (isinstance(c, str) and c.lower() == "bdeu"):
        return BDeu()
    if c is K2Score or (isinstance(c, str) and c.lower() == "k2score"):
        return K2Score()
    raise ValueError('criterion: "aic", "mdl", "bdeu", "k2score", or the AIC / MDL / BDeu / K2Score classes or instances')


def _criterion(c) -> int:
    """0 AIC, 1 MDL, 2 BDeu, 3 K2."""
    c = _canon(c)
    return {"aic": 0, "mdl": 1}[c] if isinstance(c, str) else c.kind


def _spec(c) -> _lib.ScoreSpec:
    """The family term of a criterion: kind 0 under AIC / MDL."""
    c = _canon(c)
    return _lib.ScoreSpec(0, 0, 0.0) if isinstance(c, str) else _lib.ScoreSpec(c.kind, 0, float(c.ess))


def _spec_text(kind: int, ess: float) -> str:
    return {0: "the log-likelihood term (AIC / MDL)", 2: f"BDeu(ess={ess!r})", 3: "K2"}[kind]


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    for i, x in enumerate(lists):
        ptr[i + 1] = ptr[i] + len(x)
    idx = np.array([int(v) for x in lists for v in x], dtype=np.int32)
    return ptr, idx


@contextlib.contextmanager
def _forced_splits(splits: int):
    """BN_LEARN_SPLITS = splits for the calls inside (the library reads it per call); splits <= 0 leaves the environment alone."""
    if splits <= 0:
        yield
        return
    old = os.environ.get("BN_LEARN_SPLITS")
    os.environ["BN_LEARN_SPLITS"] = str(int(splits))
    try:
        yield
    finally:
        if old is None:
            del os.environ["BN_LEARN_SPLITS"]
        else:
            os.environ["BN_LEARN_SPLITS"] = old


def score_groups(table: InfoTable, groups, counts: bool = False, splits: int = 0, criterion=None):
    """groups: [(child, base parents (strictly increasing), candidates), ...].  Returns per group the list of family terms
    [ll(base), ll(base + u_0), ...]; counts=True: (that, per group the list of uint64 count arrays in the fitted layout).
    splits > 0 fixes the number of workgroups the patterns are split over (no result depends on it).  criterion: None, "aic" or
    "mdl" give the log-likelihood term; BDeu / K2Score the Bayesian-Dirichlet term (bn_learn_score_groups_spec)."""
    spec = None if criterion is None else _spec(criterion)
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
    with _forced_splits(splits):
        args = (len(groups), _p(child, ctypes.c_int32), _p(bptr, ctypes.c_int32), _p(bidx, ctypes.c_int32), _p(cptr, ctypes.c_int32),
                _p(cidx, ctypes.c_int32), _p(ll, ctypes.c_double), _p(N, ctypes.c_uint64) if counts else None)
        if spec is None:
            _lib.check(_lib.lib().bn_learn_score_groups(table._h, *args))
        else:
            _lib.check(_lib.lib().bn_learn_score_groups_spec(table._h, ctypes.byref(spec), *args))
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


def score_subsets(table: InfoTable, child: int, base, cand, counts: bool = False, splits: int = 0, criterion=None):
    """The family terms of `child` with the parents base + S for every subset S of `cand`: a list of 2^m values, entry `mask`
    standing for S = {cand[j] : bit j of mask}.  counts=True: (that, the list of the 2^m uint64 count arrays in the fitted
    layout).  One count of the top family base + cand; every other family is summed out of it on the device.  criterion: as
    score_groups'."""
    spec = None if criterion is None else _spec(criterion)
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
    with _forced_splits(splits):
        args = (int(child), len(base), _p(base, ctypes.c_int32), m, _p(cand, ctypes.c_int32), _p(ll, ctypes.c_double),
                _p(N, ctypes.c_uint64) if counts else None)
        if spec is None:
            _lib.check(_lib.lib().bn_learn_score_subsets(table._h, *args))
        else:
            _lib.check(_lib.lib().bn_learn_score_subsets_spec(table._h, ctypes.byref(spec), *args))
    if not counts:
        return ll.tolist()
    blocks, at = [], 0
    for x in sizes:
        blocks.append(N[at:at + x])
        at += x
    return ll.tolist(), blocks


class Learner:
    """bn_learner: a graph over the columns of `table`, its family terms and its score.  `structure`: None (no edges), a
    FlatModel, per-node parent lists, or the pair (in_ptr [n + 1], in_idx) that `structure()` returns.  `criterion`: see the module's text; `info("criterion")` gives 0 AIC, 1 MDL, 2 BDeu, 3 K2."""

    def __init__(self, table: InfoTable, structure=None, criterion="aic", max_parents: int = MAX_PARENTS):
        if structure is None:
            parents = [[] for _ in range(table.n)]
        elif isinstance(structure, FlatModel):
            parents = [structure.parents(v).tolist() for v in range(structure.n)]
        elif isinstance(structure, tuple) and len(structure) == 2 and len(structure[0]) == table.n + 1:   # (in_ptr, in_idx)
            ptr, idx = structure
            parents = [[int(u) for u in idx[ptr[v]:ptr[v + 1]]] for v in range(table.n)]
        else:
            parents = [list(p) for p in structure]
        if len(parents) != table.n:
            raise ValueError(f"the structure has {len(parents)} nodes, the table {table.n} columns")
        ptr, idx = _csr(parents)
        self.table, self.n = table, table.n
        self.criterion = _canon(criterion)
        spec = _spec(self.criterion)
        self.spec = (spec.kind, spec.ess)   # the family term: what a term table must hold for anneal / hc
        h = ctypes.c_void_p()
        if spec.kind == 0:
            _lib.check(_lib.lib().bn_learn_create(table._h, _p(ptr, ctypes.c_int32), _p(idx, ctypes.c_int32), _criterion(self.criterion),
                                                  int(max_parents), ctypes.byref(h)))
        else:
            _lib.check(_lib.lib().bn_learn_create_spec(table._h, _p(ptr, ctypes.c_int32), _p(idx, ctypes.c_int32), spec.kind,
                                                       ctypes.byref(spec), int(max_parents), ctypes.byref(h)))
        self._h = h

    def _check_terms(self, term_table: "TermTable") -> None:
        if term_table.spec != self.spec:
            raise ValueError(f"the term table holds {_spec_text(*term_table.spec)} terms, the learner scores by {_spec_text(*self.spec)}")

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

    def _search(self, call, term_table: "TermTable", p, runs: int, seed: int, names, trace_dtype, cap: int, tracing: bool):
        """The plumbing of the searches over a term table: the per-run score, counts [runs][len(names)] and masks, the trace
        buffer and the winner, around call(head, score, counts, masks, trace, winner) -- the library call, `head` being its first
        five arguments.  Returns (the records every search has: names' columns, masks, winner; the scores; the trace buffer)."""
        c = max(runs, 1)
        score = np.zeros(c)
        counts = np.zeros((c, len(names)), dtype=np.uint32)
        masks = np.zeros((c, max(self.n, 1)), dtype=np.uint64)
        trace = np.zeros(max(cap, 1), dtype=trace_dtype)
        winner = ctypes.c_int32()
        head = (self._h, term_table._h, ctypes.byref(p), runs, int(seed) & (2 ** 64 - 1))
        _lib.check(call(head, _p(score, ctypes.c_double), _p(counts, ctypes.c_uint32), _p(masks, ctypes.c_uint64),
                        trace.ctypes.data if tracing else None, ctypes.byref(winner)))
        out = {name: counts[:, i].copy() for i, name in enumerate(names)}
        out.update({"masks": masks[:, :self.n], "winner": winner.value})
        return out, score, trace

    def anneal(self, term_table: "TermTable", initial_temp: float, final_temp: float, decreasing_rate: float, boltzmann: float = 1.0,
               same_state_max: int = 100, chains: int = 64, seed: int = 0, rule: str = "reference", max_proposals: int = 1 << 20,
               trace_chain=None, trace_cap=None) -> dict:
        """simulated_annealing::operator() as `chains` independent chains on the device, each from this learner's graph; the
        chain with the strictly smallest final evaluation (the lowest index among equals) becomes this learner's graph.
        rule: "reference" (accept uphill iff u < exp(-now / (boltzmann * T))) or "metropolis" (exp(-diff / ...)).  Returns the
        per-chain records: eval [chains], proposals / operated / accepted / flags [chains] (END_* bits), masks [chains][n]
        (bit u of masks[j][v]: u -> v), edges: per chain the ordered list of (from, to), winner, and with trace_chain the
        structured array `trace` (TRACE_DTYPE) of that chain's operated proposals (the first trace_cap, default max_proposals)."""
        if rule not in _RULES:
            raise ValueError('rule: "reference" or "metropolis"')
        self._check_terms(term_table)
        chains = int(chains)
        tracing = trace_chain is not None
        cap = int(max_proposals if trace_cap is None else trace_cap) if tracing else 0
        p = _lib.AnnealParams(float(initial_temp), float(final_temp), float(decreasing_rate), float(boltzmann), int(same_state_max),
                              int(max_proposals), _RULES[rule], int(trace_chain) if tracing else -1, cap, 0)
        n_edges = np.zeros(max(chains, 1), dtype=np.int32)
        edges = np.zeros((max(chains, 1), max(self.n * term_table.max_parents, 1)), dtype=np.uint16)
        out, ev, trace = self._search(
            lambda head, ev, counts, masks, trace, winner: _lib.lib().bn_learn_anneal(
                *head, ev, counts, masks, _p(n_edges, ctypes.c_int32), _p(edges, ctypes.c_uint16), trace, winner),
            term_table, p, chains, seed, ("proposals", "operated", "accepted", "flags"), TRACE_DTYPE, cap, tracing)
        out.update({"eval": ev, "edges": [[(int(e) & 255, int(e) >> 8) for e in edges[j, :n_edges[j]]] for j in range(chains)]})
        if tracing:
            out["trace"] = trace[:min(int(out["operated"][int(trace_chain)]), cap)].copy()
        return out

    def hc(self, term_table: "TermTable", alpha: float, runs: int = 64, seed: int = 0, max_parents=None, similarity=None,
           trace_run=None, trace_cap: int = 2048) -> dict:
        """stepwise_structure_hc::operator() as `runs` independent runs on the device, each from the empty graph (the algorithm
        clears the edges); the run with the strictly smallest final score (the lowest among equals) becomes this learner's graph.
        similarity: None (the table's all-pairs mutual information) or an [n][n] matrix, symmetric in bits.  max_parents: the
        in-degree a run refuses at (default and at most the term table's).  Returns the per-run records: score [runs], merges /
        tried / kept / pruned / pairs_kept / flags [runs] (HC_* bits), masks [runs][n] (bit u of masks[j][v]: u -> v), winner, and
        with trace_run the structured arrays `merge_trace` (parent, child, value_bits, coin) and `prune_trace` (cluster,
        connections, value_bits, pruned) of that run."""
        runs = int(runs)
        self._check_terms(term_table)
        tracing = trace_run is not None
        cap = int(trace_cap) if tracing else 0
        p = _lib.HcParams(float(alpha), int(term_table.max_parents if max_parents is None else max_parents),
                          int(trace_run) if tracing else -1, cap, 0)
        S = None
        if similarity is not None:
            S = np.ascontiguousarray(similarity, dtype=np.float64)
            if S.shape != (self.n, self.n):
                raise ValueError(f"similarity: an [{self.n}][{self.n}] matrix")
        n_trace = ctypes.c_int32()
        out, score, trace = self._search(
            lambda head, score, counts, masks, trace, winner: _lib.lib().bn_learn_hc(
                *head, _p(S, ctypes.c_double) if S is not None else None, score, counts, masks, trace, ctypes.byref(n_trace), winner),
            term_table, p, runs, seed, ("merges", "tried", "kept", "pruned", "pairs_kept", "flags"), HC_TRACE_DTYPE, cap, tracing)
        out["score"] = score
        if tracing:
            tr = trace[:n_trace.value]
            merge, visit = tr[tr["kind"] == 0], tr[tr["kind"] == 1]
            out["merge_trace"] = np.rec.fromarrays([merge["a"], merge["b"], merge["value_bits"], merge["c"]], names="parent,child,value_bits,coin")
            out["prune_trace"] = np.rec.fromarrays([visit["a"], visit["b"], visit["value_bits"], visit["c"]],
                                                   names="cluster,connections,value_bits,pruned")
        return out

    def climb(self, term_table: "TermTable", tabu_len: int = 0, max_worse: int = 0, runs: int = 1, perturb: int = 0, seed: int = 0,
              max_parents=None, max_steps: int = 0, trace_run=None, trace_cap: int = 0) -> dict:
        """Tabu hill climbing (bn_learn_climb) as `runs` independent runs on the device: steepest descent over the add, delete
        and reverse moves, a move on a node pair tabu for `tabu_len` applied steps, up to `max_worse` steps in a row without a new
        best.  Run 0 starts from this learner's graph, run j >= 1 from that graph after `perturb` random proposals of stream (seed,
        j).  The best graph of the run with the strictly smallest score (the lowest among equals) becomes this learner's graph.
        max_parents: the in-degree a run refuses at (default and at most the term table's); max_steps 0: 2^16.  Returns the per-run
        records: score [runs], steps / improving / perturbed / best_step / flags / tabu_legal [runs] (CLIMB_* bits), masks
        [runs][n] (bit u of masks[j][v]: u -> v), winner, and with trace_run the structured array `trace` (CLIMB_TRACE_DTYPE) of
        that run's applied steps (the first trace_cap; 0: max_steps)."""
        runs = int(runs)
        self._check_terms(term_table)
        tracing = trace_run is not None
        cap = (int(trace_cap) or int(max_steps) or (1 << 16)) if tracing else 0
        p = _lib.ClimbParams(int(term_table.max_parents if max_parents is None else max_parents), int(tabu_len), int(max_worse), int(max_steps),
                             int(perturb), int(trace_run) if tracing else -1, cap, 0)
        out, score, trace = self._search(
            lambda head, *outputs: _lib.lib().bn_learn_climb(*head, *outputs), term_table, p, runs, seed,
            ("steps", "improving", "perturbed", "best_step", "flags", "tabu_legal"), CLIMB_TRACE_DTYPE, cap, tracing)
        out["score"] = score
        if tracing:
            out["trace"] = trace[:min(int(out["steps"][int(trace_run)]), cap)].copy()
        return out

    def optimal(self, term_table: "TermTable", max_parents=None, allowed=None) -> dict:
        """The exact search (bn_learn_optimal): a DAG of the globally smallest sum of family costs within the in-degree bound, by
        dynamic programming over node subsets; at most 24 nodes.  It becomes this learner's graph; the starting graph is not read.
        max_parents: the in-degree bound (default and at most the term table's).  allowed: None, per-node lists of the nodes that
        may be parents, per-node masks (bit u of allowed[v]: u may be a parent of v), an [n][n] adjacency matrix, or a PCResult
        (its skeleton).  Returns value (the cost of the graph as the search added it up: R[V]), order (a topological order, parents
        first), masks [n] (bit u of masks[v]: u -> v) and parents (per-node lists)."""
        self._check_terms(term_table)
        n = self.n
        words = None
        if allowed is not None:
            words = _allowed_masks(allowed, n)
        p = _lib.OptimalParams(int(term_table.max_parents if max_parents is None else max_parents), 0,
                               _p(words, ctypes.c_uint64) if words is not None else None, 0)
        value = ctypes.c_double()
        order = np.zeros(max(n, 1), dtype=np.int32)
        masks = np.zeros(max(n, 1), dtype=np.uint64)
        _lib.check(_lib.lib().bn_learn_optimal(self._h, term_table._h, ctypes.byref(p), ctypes.byref(value), _p(order, ctypes.c_int32),
                                               _p(masks, ctypes.c_uint64)))
        masks = masks[:n]
        return {"value": value.value, "order": order[:n], "masks": masks,
                "parents": [[u for u in range(n) if (int(m) >> u) & 1] for m in masks]}

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


def _allowed_masks(allowed, n: int) -> np.ndarray:
    """Learner.optimal's `allowed` as [n] uint64 masks: a PCResult (its skeleton), an [n][n] matrix of marks, per-node lists of
    node ids, or per-node masks (n integers)."""
    if hasattr(allowed, "skeleton"):
        allowed = allowed.skeleton
    if isinstance(allowed, np.ndarray) and allowed.ndim == 2:
        if allowed.shape != (n, n):
            raise ValueError(f"allowed: an [{n}][{n}] matrix")
        return np.array([sum(1 << u for u in range(n) if allowed[v, u]) for v in range(n)], dtype=np.uint64)
    if len(allowed) != n:
        raise ValueError(f"allowed: one entry per node ({n})")
    words = np.zeros(n, dtype=np.uint64)
    for v, a in enumerate(allowed):
        if isinstance(a, (int, np.integer)):
            words[v] = int(a)
        else:
            ids = [int(u) for u in a]
            if any(not 0 <= u < 64 for u in ids):
                raise ValueError("allowed: node ids within 0 .. 63")
            words[v] = sum(1 << u for u in set(ids))
    return words


TRACE_DTYPE = np.dtype([("now_bits", np.uint64), ("method", np.uint8), ("from", np.uint8), ("to", np.uint8), ("accepted", np.uint8),
                        ("pad", np.uint32)])
END_TEMPERATURE, END_SAME_STATE, END_CAP = 1, 2, 4   # flags of a chain's record
_RULES = {"reference": 0, "metropolis": 1}
HC_TRACE_DTYPE = np.dtype([("value_bits", np.uint64), ("kind", np.uint8), ("a", np.uint8), ("b", np.uint8), ("c", np.uint8), ("pad", np.uint32)])
HC_ONE_CLUSTER, HC_NO_SIMILARITY = 1, 2   # flags of a run's record
CLIMB_TRACE_DTYPE = np.dtype([("d_bits", np.uint64), ("current_bits", np.uint64), ("kind", np.uint8), ("from", np.uint8), ("to", np.uint8),
                              ("pad8", np.uint8), ("pad32", np.uint32), ("pad", np.uint64)])
CLIMB_NO_MOVE, CLIMB_LOCAL_OPTIMUM, CLIMB_CAP = 1, 2, 4   # flags of a hill-climbing run's record


class TermTable:
    """bn_term_table: ll(c, S) for every child c and every parent set S of at most `max_parents` nodes other than c, resident
    on the device, each entry bit for bit what `score_groups` gives for that family (NaN: a family over 2^20 table entries, not
    eligible).  At most 64 nodes and n * T(n, q) <= 2^22 entries.  `row(child)` fetches one child's T(n, q) entries, `rank(child,
    parents)` is the index of a parent set in it.  Borrows `table`: close the term table first."""

    def __init__(self, table: InfoTable, max_parents: int = 3, criterion=None):
        h = ctypes.c_void_p()
        spec = _lib.ScoreSpec(0, 0, 0.0) if criterion is None else _spec(criterion)
        if criterion is None:
            _lib.check(_lib.lib().bn_terms_create(table._h, int(max_parents), ctypes.byref(h)))
        else:
            _lib.check(_lib.lib().bn_terms_create_spec(table._h, ctypes.byref(spec), int(max_parents), ctypes.byref(h)))
        self._h = h
        self.spec = (spec.kind, spec.ess)
        self.table, self.n, self.max_parents = table, table.n, int(max_parents)
        self.row_entries = self.info("row_entries")

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().bn_terms_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self, name: str) -> int:
        out = ctypes.c_int64()
        _lib.check(_lib.lib().bn_terms_get(self._h, name.encode(), ctypes.byref(out)))
        return out.value

    def row(self, child: int) -> np.ndarray:
        out = np.zeros(self.row_entries)
        _lib.check(_lib.lib().bn_terms_fetch(self._h, int(child), _p(out, ctypes.c_double)))
        return out

    def rank(self, child: int, parents) -> int:
        """offset[j] + sum_i C(s'_i, i) over the parents relabelled s' = s - (s > child), in increasing order, i = 1 .. j."""
        from math import comb
        ps = sorted(int(u) for u in parents)
        if len(ps) > self.max_parents or len(set(ps)) != len(ps) or any(u == child or not 0 <= u < self.n for u in ps):
            raise ValueError("parents: distinct nodes other than the child, at most max_parents of them")
        r = sum(comb(self.n - 1, t) for t in range(len(ps)))
        return r + sum(comb(u - (u > child), i + 1) for i, u in enumerate(ps))


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
        self._name = _canon(criterion)   # what is passed on to Learner, TermTable and the inner searches
        self._rng = np.random.default_rng(seed)
        self._table = sampling if isinstance(sampling, InfoTable) else None
        self.last = {}   # counters of the last search: families_scored, passes, count_ns, score_ns, lattice_ns, subsets_scored

    def _ensure_table(self, model) -> InfoTable:
        if self._table is None:
            self._table = table_from_sampler(self._sampling, range(model.n), model.k, self._device)
        return self._table

    def _learner(self, model) -> Learner:
        return Learner(self._ensure_table(model), model, self._name, self._max_parents)

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
        return kind(self._name, self._table, max_parents=self._max_parents, seed=seed, device=self._device)

    def __call__(self, model, initial_cluster_size: int, plan=None):
        size = int(initial_cluster_size)
        if size <= 0:
            raise ValueError("initial_cluster_size must be positive")
        table = self._ensure_table(model)
        inner, between = self._make(self._inner), self._make(self._between)
        with Learner(table, None, self._name, self._max_parents) as L:   # (:26: erase_all_edge)
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


class _TermSearch(_Search):
    """What the searches over a term table share: the table, kept for the object's lifetime; the seed of call number i, seed + i
    (without a seed one is drawn); `records`, the Learner method's records of the last call on the device."""

    def __init__(self, criterion, sampling, max_parents, seed, device):
        super().__init__(criterion, sampling, max_parents, seed, device)
        self._seed = int(self._rng.integers(1 << 62)) if seed is None else int(seed)
        self._calls = 0
        self._terms = None
        self.records = None

    def close(self) -> None:
        if getattr(self, "_terms", None) is not None:
            self._terms.close()
            self._terms = None

    __del__ = close

    def term_table(self, model) -> TermTable:
        if self._terms is None:
            self._terms = TermTable(self._ensure_table(model), self._max_parents, self._name)
        return self._terms

    def _next_seed(self) -> int:
        self._calls += 1
        return self._seed + self._calls - 1

    def _note(self, L: Learner, terms: TermTable, names) -> None:
        """`last` gains the search's counters `names`, the winner and the term table's counters."""
        self.last.update({name: L.info(name) for name in names})
        self.last.update({"winner": self.records["winner"], "term_entries": terms.info("entries"), "term_passes": terms.info("passes"),
                          "term_families_scored": terms.info("families_scored"), "term_build_ns": terms.info("build_ns")})


class SimulatedAnnealing(_TermSearch):
    """bn::learning::simulated_annealing<Eval> (simulated_annealing.hpp).  `sa(model, initial_temp, final_temp, decreasing_rate,
    boltzmann=1.0, same_state_max=100)`: `chains` independent chains from the model's graph, the best final graph returned as
    (FlatModel with CPTs fitted to it, score).  max_parents (default 3) bounds the in-degree: the family terms of every parent
    set up to it are computed once, into a TermTable kept for the object's lifetime, so a second call on the same samples pays
    only for the chains.  rule: "reference" or "metropolis" (Learner.anneal).  Chain j of call number i uses the stream (seed +
    i, j); without a seed one is drawn.  `last` also holds the anneal counters, the winning chain and the term table's."""

    def __init__(self, criterion, sampling, max_parents: int = 3, chains: int = 64, rule: str = "reference", seed=None,
                 max_proposals: int = 1 << 20, device: int = _lib.BN_DEVICE_CURRENT):
        super().__init__(criterion, sampling, max_parents, seed, device)
        self._chains, self._rule, self._max_proposals = int(chains), rule, int(max_proposals)

    def __call__(self, model, initial_temp: float, final_temp: float, decreasing_rate: float, boltzmann: float = 1.0,
                 same_state_max: int = 100):
        terms = self.term_table(model)
        with self._learner(model) as L:
            self.records = L.anneal(terms, initial_temp, final_temp, decreasing_rate, boltzmann, same_state_max, self._chains,
                                    self._next_seed(), self._rule, self._max_proposals)
            out = self._finish(model, L)
            self._note(L, terms, ("anneal_ns", "anneal_chains", "anneal_steps"))
            return out


class HillClimbing(_TermSearch):
    """Tabu hill climbing over add, delete and reverse moves (Learner.climb; the search of bnlearn's hc / tabu and pgmpy's
    HillClimbSearch, not in the reference).  `hc(model, tabu_len=0, max_worse=0, perturb=0, max_steps=0)`: `runs` independent runs,
    run 0 from the model's graph and the others from perturbed copies of it, the best graph returned as (FlatModel with CPTs
    fitted to it, score).  max_parents (default 3) bounds the in-degree: the family terms of every parent set up to it are computed
    once, into a TermTable kept for the object's lifetime.  Run j of call number i uses the stream (seed + i, j); without a seed one
    is drawn.  `last` also holds the climb counters, the winning run and the term table's."""

    def __init__(self, criterion, sampling, max_parents: int = 3, runs: int = 1, seed=None, device: int = _lib.BN_DEVICE_CURRENT):
        super().__init__(criterion, sampling, max_parents, seed, device)
        self._runs = int(runs)

    def __call__(self, model, tabu_len: int = 0, max_worse: int = 0, perturb: int = 0, max_steps: int = 0):
        terms = self.term_table(model)
        with self._learner(model) as L:
            self.records = L.climb(terms, tabu_len, max_worse, self._runs, perturb, self._next_seed(), max_steps=max_steps)
            out = self._finish(model, L)
            self._note(L, terms, ("climb_ns", "climb_runs", "climb_steps"))
            return out


class OptimalSearch(_TermSearch):
    """The exact search (Learner.optimal; Silander & Myllymaki's dynamic programming over node subsets, the search of pgmpy's
    ExhaustiveSearch, not in the reference).  `opt(model, allowed=None)`: the DAG of the globally smallest score within the in-degree
    bound, returned as (FlatModel with CPTs fitted to it, score); the model's own graph is not read.  At most 24 nodes.  max_parents
    (default 3) bounds the in-degree: the family terms of every parent set up to it are computed once, into a TermTable kept for the
    object's lifetime.  allowed: as Learner.optimal's (a PC result's skeleton restricts the search to it).  `records` holds
    Learner.optimal's result, `last` also the search's counters and the term table's."""

    def __init__(self, criterion, sampling, max_parents: int = 3, device: int = _lib.BN_DEVICE_CURRENT):
        super().__init__(criterion, sampling, max_parents, 0, device)

    def __call__(self, model, allowed=None):
        terms = self.term_table(model)
        with self._learner(model) as L:
            self.records = L.optimal(terms, allowed=allowed)
            self.records["winner"] = 0
            out = self._finish(model, L)
            self._note(L, terms, ("optimal_ns", "optimal_bps_ns", "optimal_sink_ns", "optimal_cells", "optimal_bytes"))
            return out


class _Stream:
    """The library's stream (run j of a seed): xoshiro128++ seeded by Philox4x32-10({j_lo, j_hi, 0, 0}, {seed_lo, seed_hi})."""

    def __init__(self, seed: int, j: int):
        M = 0xFFFFFFFF
        c = [j & M, (j >> 32) & M, 0, 0]
        k0, k1 = seed & M, (seed >> 32) & M
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M, (p0 >> 32) ^ c[3] ^ k1, p0 & M]
            k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
        self.x = c if any(c) else [1, 0, 0, 0]

    def next(self) -> int:
        M = 0xFFFFFFFF
        x = self.x
        s = (x[0] + x[3]) & M
        result = ((((s << 7) | (s >> 25)) & M) + x[0]) & M
        t = (x[1] << 9) & M
        x[2] ^= x[0]
        x[3] ^= x[1]
        x[1] ^= x[2]
        x[0] ^= x[3]
        x[2] ^= t
        x[3] = ((x[3] << 11) | (x[3] >> 21)) & M
        return result

    def below(self, m: int) -> int:
        return (self.next() * m) >> 32

    def uniform(self) -> float:
        return (self.next() + 0.5) * 2.0 ** -32


class StepwiseStructureHC(_TermSearch):
    """bn::learning::stepwise_structure_hc<Eval, BetweenLearning> (stepwise_structure_hc.hpp): nodes are clustered by mutual
    information; the two most similar clusters are merged, edges from the one to the other learned with `learn_with_hint`, and the
    merged cluster's pairs with the others pruned at random (`alpha`: 0 prunes nothing, 1 everything).  `hc(model, alpha)` returns
    (FlatModel with CPTs fitted to the final structure, score); the model's edges are not read (the algorithm clears them).
    between unset or Greedy: `runs` independent runs resident on the device (Learner.hc), the best final graph returned; run j of
    call number i uses the stream (seed + i, j).  The term table (max_parents, default 3) is kept for the object's lifetime.
    Any other `between` (BruteForce, or anything with `hint_on`, class or instance): the same loop on the host as ONE run, coin
    and pruning draws from run 0's stream, `between.hint_on(L, parent_nodes, child_nodes)` per merge.  Clusters are ordered by id
    where the reference orders them by address: node i's cluster is i, merge s makes n + s.  With nothing to merge the score is
    the empty graph's (the reference returns DBL_MAX).  `last` also holds the hc counters, the winner and the term table's."""

    def __init__(self, criterion, sampling, between=None, max_parents: int = 3, runs: int = 64, seed=None,
                 device: int = _lib.BN_DEVICE_CURRENT):
        super().__init__(criterion, sampling, max_parents, seed, device)
        self._between = Greedy if between is None else between
        self._runs = int(runs)
        self._seeded = seed is not None

    def _resident(self) -> bool:
        return self._between is Greedy or isinstance(self._between, Greedy)

    def __call__(self, model, alpha: float):
        table = self._ensure_table(model)
        seed = self._next_seed()
        with Learner(table, None, self._name, self._max_parents) as L:   # (:134: erase_all_edge)
            if self._resident():
                terms = self.term_table(model)
                self.records = L.hc(terms, alpha, self._runs, seed)
                out = self._finish(model, L)
                self._note(L, terms, ("hc_ns", "hc_runs", "hc_merges"))
                return out
            merges = self._host_run(L, table, float(alpha), seed)
            out = self._finish(model, L)
            self.last.update({"hc_runs": 1, "hc_merges": merges, "winner": 0})
            return out

    def _host_run(self, L: Learner, table: InfoTable, alpha: float, seed: int) -> int:
        between = self._between
        if isinstance(between, type):
            between = between(self._name, table, max_parents=self._max_parents,
                              seed=int(self._rng.integers(1 << 32)) if self._seeded else None, device=self._device)
        n = L.n
        S = table.pair_entropies()["mi"]
        rng = _Stream(seed, 0)
        f = np.float64

        def make_similarity(X, Y):   # (:240-259)
            count, value = f(len(X) * len(Y)), f(0.0)
            for l in X:
                for r in Y:
                    value = value + S[l][r] / count
            return value

        with np.errstate(all="ignore"):
            nodes = {i: [i] for i in range(n)}
            clusters = list(range(n))
            sims = []
            average = f(0.0)
            for i in range(n):
                for j in range(i + 1, n):
                    value = make_similarity([i], [j])
                    average = average + value / f(n * (n - 1) // 2)
                    sims.append((i, j, value))
            merges = 0
            while len(clusters) != 1 and sims:   # (:267)
                best = 0
                for i in range(1, len(sims)):
                    if sims[best][2] < sims[i][2]:
                        best = i
                a, b, old_value = sims.pop(best)
                parent, child = (b, a) if rng.below(2) else (a, b)
                between.hint_on(L, list(nodes[parent]), list(nodes[child]))
                new = n + merges
                merges += 1
                nodes[new] = nodes[parent] + nodes[child]
                clusters.remove(parent)
                clusters.remove(child)
                clusters.append(new)
                dead = (parent, child)
                for c in clusters[:-1]:   # (:299-348)
                    connection = [s for s in sims if (s[0] == c and s[1] in dead) or (s[1] == c and s[0] in dead)]
                    sims = [s for s in sims if not ((s[0] == c and s[1] in dead) or (s[1] == c and s[0] in dead))]
                    new_value = make_similarity(nodes[new], nodes[c])
                    if len(connection) == 2:
                        p = np.power(f(alpha), new_value / average)
                    elif len(connection) == 1:
                        p = np.power(f(alpha), old_value / connection[0][2])
                    else:
                        continue
                    if rng.uniform() < p:
                        continue
                    sims.append((c, new, new_value))
        return merges


# ---- constraint-based learning: PC-stable (bn_learn_pc, bn_pdag_to_dag) ------------------------------

class PCResult:
    """skeleton, cpdag: [n][n] uint8 marks (both [a][b] and [b][a] set: a - b; only [a][b]: a -> b); sepsets: {(a, b) with a < b:
    tuple S} for every removed edge; levels: per level {"tests", "removed", "count_ns", "stat_ns"}; tests_skipped: tests over the
    2^20-cell limit (not run, dependent)."""

    def __init__(self, skeleton, cpdag, sepsets, levels, tests_skipped):
        self.skeleton, self.cpdag, self.sepsets, self.levels, self.tests_skipped = skeleton, cpdag, sepsets, levels, tests_skipped

    def dag(self):
        """Per-node parent lists of a consistent DAG extension of the cpdag."""
        return cpdag_to_dag(self.cpdag)


def cpdag_to_dag(cpdag):
    """A consistent DAG extension of a PDAG mark matrix (Dor-Tarsi, the lowest eligible node first) as per-node parent lists,
    parents increasing: what `Learner(table, structure=...)` takes.  No extension: BnError (BN_ERR_STATE)."""
    m = np.ascontiguousarray(cpdag, dtype=np.uint8)
    n = m.shape[0]
    if m.shape != (n, n):
        raise ValueError("cpdag must be [n][n]")
    ptr = np.zeros(n + 1, dtype=np.int32)
    idx = np.zeros(max(n * (n - 1) // 2, 1), dtype=np.int32)
    _lib.check(_lib.lib().bn_pdag_to_dag(n, _p(m, ctypes.c_uint8), _p(ptr, ctypes.c_int32), _p(idx, ctypes.c_int32)))
    return [idx[ptr[v]:ptr[v + 1]].tolist() for v in range(n)]


class PC:
    """PC-stable under the G^2 test: `PC(alpha, max_cond, df_rule)(table_or_model, start=None)`.  A test is independent iff its
    p-value > alpha; levels |S| = 0 .. max_cond (at most 8); df_rule "nominal" (bnlearn mi) or "adjusted" (mi-adf).  `sampling` (an
    InfoTable or an engine.Sampler) is needed when the call is given a model instead of a table; `start` is a symmetric [n][n]
    adjacency to begin from instead of the complete graph.  max_tests: the per-level cap (0: the library's default, 2^22)."""

    def __init__(self, alpha: float = 0.05, max_cond: int = 3, df_rule="nominal", sampling=None, max_tests: int = 0,
                 device: int = _lib.BN_DEVICE_CURRENT):
        from .evaluation import _df_rule
        self.alpha, self.max_cond, self.df_rule, self.max_tests = float(alpha), int(max_cond), _df_rule(df_rule), int(max_tests)
        self._sampling, self._device = sampling, device

    def __call__(self, table_or_model, start=None) -> PCResult:
        if isinstance(table_or_model, InfoTable):
            table = table_or_model
        elif isinstance(self._sampling, InfoTable):
            table = self._sampling
        elif self._sampling is not None:
            table = table_from_sampler(self._sampling, range(table_or_model.n), table_or_model.k, self._device)
        else:
            raise ValueError("PC: give an InfoTable, or a model with PC(sampling=...)")
        n, mc = table.n, self.max_cond
        params = _lib.PcParams(self.alpha, mc, self.df_rule, self.max_tests)
        st = None
        if start is not None:
            st = np.ascontiguousarray(np.asarray(start) != 0, dtype=np.uint8)
            if st.shape != (n, n):
                raise ValueError("start must be [n][n]")
        skel, cpdag = np.zeros((n, n), dtype=np.uint8), np.zeros((n, n), dtype=np.uint8)
        sep_len = np.full((n, n), -1, dtype=np.int32)
        sep_idx = np.zeros((n, n, max(mc, 1)), dtype=np.int32)
        levels = (_lib.PcLevel * (max(mc, 0) + 1))()
        n_levels, skipped = ctypes.c_int32(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().bn_learn_pc(table._h, ctypes.byref(params), _p(st, ctypes.c_uint8) if st is not None else None,
                                          _p(skel, ctypes.c_uint8), _p(cpdag, ctypes.c_uint8), _p(sep_len, ctypes.c_int32),
                                          _p(sep_idx, ctypes.c_int32) if mc > 0 else None, levels, ctypes.byref(n_levels),
                                          ctypes.byref(skipped)))
        sepsets = {(a, b): tuple(int(v) for v in sep_idx[a, b, :sep_len[a, b]])
                   for a in range(n) for b in range(a + 1, n) if sep_len[a, b] >= 0}
        recs = [{"tests": int(levels[i].tests), "removed": int(levels[i].removed), "count_ns": float(levels[i].count_ns),
                 "stat_ns": float(levels[i].stat_ns)} for i in range(n_levels.value)]
        return PCResult(skel, cpdag, sepsets, recs, int(skipped.value))


# ---- tree learners: Chow-Liu and tree-augmented naive Bayes (bn_learn_tree, bn_tree_max_spanning) ----

def max_spanning_tree(w, root: int = 0, device: int = _lib.BN_DEVICE_CURRENT) -> np.ndarray:
    """parent [m] (int32, -1 at `root`) of the maximum spanning tree of the weights w [m][m] under the library's edge order: weight
    descending, then (min, max) of the end points ascending.  Only the upper triangle is read."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    m = w.shape[0]
    if w.ndim != 2 or w.shape != (m, m):
        raise ValueError("w must be [m][m]")
    parent = np.zeros(max(m, 1), dtype=np.int32)
    _lib.check(_lib.lib().bn_tree_max_spanning(m, _p(w, ctypes.c_double), int(root), device, _p(parent, ctypes.c_int32)))
    return parent[:m]


class TreeResult:
    """variables [m]: the columns of the tree; parent [m]: the parent column of variables[i], -1 at the root; weight [m]: the matrix
    entry of that edge, 0.0 at the root; matrix [m][m]: the mutual information (Chow-Liu) or the mutual information given the class
    (TAN) of the variables; root: the root column; cond: the class column, -1 for Chow-Liu; n: the table's columns."""

    def __init__(self, n, variables, parent, weight, matrix, root, cond):
        self.n, self.variables, self.parent, self.weight, self.matrix, self.root, self.cond = n, variables, parent, weight, matrix, root, cond

    def parents(self):
        """Per column of the table the sorted list of its parents: the tree parent and, for TAN, the class."""
        out = [[] for _ in range(self.n)]
        for v, p in zip(self.variables, self.parent):
            ps = ([int(p)] if p >= 0 else []) + ([self.cond] if self.cond >= 0 else [])
            out[int(v)] = sorted(ps)
        return out

    def structure(self):
        """(in_ptr, in_idx): what `Learner(table, structure=...)` and `structure_model` take."""
        return _csr(self.parents())


class _TreeLearner:
    def __init__(self, sampling=None, root=None, device: int = _lib.BN_DEVICE_CURRENT):
        self._sampling, self.root, self._device = sampling, root, device

    def _run(self, table_or_model, what, cond, variables) -> TreeResult:
        if isinstance(table_or_model, InfoTable):
            return self._learn(table_or_model, cond, variables)
        if isinstance(self._sampling, InfoTable):
            return self._learn(self._sampling, cond, variables)
        if self._sampling is None:
            raise ValueError(f"{what}: give an InfoTable, or a model with {what}(sampling=...)")
        # a sampler: the table made from it lives for this call only
        with table_from_sampler(self._sampling, range(table_or_model.n), table_or_model.k, self._device) as table:
            return self._learn(table, cond, variables)

    def _learn(self, table, cond, variables) -> TreeResult:
        if variables is None:
            variables = [v for v in range(table.n) if v != cond]
        v = np.ascontiguousarray(variables, dtype=np.int32).reshape(-1)
        m = len(v)
        parent, weight = np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1))
        matrix = np.zeros((max(m, 1), max(m, 1)))
        root = -1 if self.root is None else int(self.root)
        _lib.check(_lib.lib().bn_learn_tree(table._h, cond, m, _p(v, ctypes.c_int32), root, _p(parent, ctypes.c_int32),
                                            _p(weight, ctypes.c_double), _p(matrix, ctypes.c_double)))
        return TreeResult(table.n, v, parent[:m], weight[:m], matrix[:m, :m], int(v[parent[:m] < 0][0]), cond)


class ChowLiu(_TreeLearner):
    """The Chow-Liu tree (bnlearn chow.liu, pgmpy TreeSearch "chow-liu"): `ChowLiu(sampling=None, root=None)(table_or_model,
    variables=None)` is the maximum spanning tree of the all-pairs mutual information, oriented away from `root` (None: the lowest
    column).  `sampling` is needed when the call is given a model instead of a table.  Returns a TreeResult."""

    def __call__(self, table_or_model, variables=None) -> TreeResult:
        return self._run(table_or_model, "ChowLiu", -1, variables)


class TAN(_TreeLearner):
    """Tree-augmented naive Bayes (bnlearn tree.bayes, pgmpy TreeSearch "tan"): `TAN(class_node, sampling=None, root=None)(
    table_or_model, variables=None)` is the maximum spanning tree of the features under I(X; Y | class), plus the class as a parent of
    every feature.  Returns a TreeResult."""

    def __init__(self, class_node: int, sampling=None, root=None, device: int = _lib.BN_DEVICE_CURRENT):
        super().__init__(sampling, root, device)
        self.class_node = int(class_node)

    def __call__(self, table_or_model, variables=None) -> TreeResult:
        if self.class_node < 0:
            raise ValueError("TAN: the class column must be >= 0")
        return self._run(table_or_model, "TAN", self.class_node, variables)
