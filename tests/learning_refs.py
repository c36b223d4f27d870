"""Plain Python / libm restatement of the structure-learning contract of include/bn_mi355x.h (bn_learn_*) and of the reference's
loops (bayesian/learning/greedy.hpp, k2_algorithm.hpp).

A family term here is  sum over the entries with N != 0 of double(N) * math.log(double(N) / double(row total))  in the stated
order (256 partial sums, folded by halves).  With math.log that is, bit for bit, what the public API gives for the fitted model
(bn_fit_cpt's theta = double(N) / double(total), bn_score_nodes' host logarithm and order), so `RefLearner` with `libm_ll` IS the
public-API loop (fit_cpt -> Engine -> AIC / MDL per candidate) restated on the CPU; with the device's own family terms it is the
scan of bn_learn_try_parents (contract 6)."""
import math
import os

import numpy as np

from loglik_refs import LANES, gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
MAX_PARENTS, MAX_ENTRIES = 16, 1 << 20


# ---- families ------------------------------------------------------------------------------------

def family_counts(pats, counts, k, child, parents) -> np.ndarray:
    """Exact uint64 counts of the family (child | parents) in the fitted layout: parents in increasing id, first most
    significant, the child's state least."""
    pats = np.asarray(pats).astype(np.int64)
    row = np.zeros(pats.shape[0], dtype=np.int64)
    size = int(k[child])
    for u in sorted(int(x) for x in parents):
        row = row * int(k[u]) + pats[:, u]
        size *= int(k[u])
    N = np.zeros(size, dtype=np.uint64)
    np.add.at(N, row * int(k[child]) + pats[:, child], np.asarray(counts, dtype=np.uint64))
    return N


def family_terms(N, kc, log=math.log) -> np.ndarray:
    """t[r] = double(N[r]) * log(double(N[r]) / double(row total)); 0.0 where N[r] == 0."""
    N = np.asarray(N, dtype=np.uint64).reshape(-1, int(kc))
    tot = N.sum(axis=1, dtype=np.uint64)
    t = np.zeros(N.shape)
    for r, s in zip(*np.nonzero(N)):
        n = float(N[r, s])
        t[r, s] = n * log(n / float(tot[r]))
    return t.reshape(-1)


def sum256(t) -> float:
    """bn_score_nodes' order: partial j takes the entries j, j + 256, ... from +0.0; folded by halves."""
    t = np.asarray(t, dtype=np.float64)
    pad = np.zeros((len(t) + LANES - 1) // LANES * LANES)
    pad[:len(t)] = t
    part = np.zeros(LANES)
    for chunk in pad.reshape(-1, LANES):
        part = part + chunk
    s = LANES // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return float(part[0])


def ll_bound(N, kc) -> float:
    """Contract 3: |device ll - fsum of the libm terms| <= (8u + gamma_{m+1}) * sum |t|."""
    t = family_terms(N, kc)
    m = int(np.count_nonzero(np.asarray(N)))
    return (8 * U + gamma(m + 1)) * math.fsum(np.abs(t).tolist())


class Table:
    """A pattern table on the host with a cache of family statistics: ll (libm, stated order), sum |t|, non-zero terms."""

    def __init__(self, pats, counts, k):
        self.pats = np.ascontiguousarray(pats, dtype=np.uint8)
        self.counts = np.ascontiguousarray(counts, dtype=np.uint64)
        self.k = np.asarray(k, dtype=np.int32)
        self.n = len(self.k)
        self.total = int(self.counts.sum(dtype=np.uint64))
        self._cache = {}

    def family(self, child, parents):
        key = (int(child), tuple(sorted(int(u) for u in parents)))
        if key not in self._cache:
            N = family_counts(self.pats, self.counts, self.k, key[0], key[1])
            t = family_terms(N, self.k[key[0]])
            self._cache[key] = (sum256(t), math.fsum(np.abs(t).tolist()), int(np.count_nonzero(N)))
        return self._cache[key]

    def libm_ll(self, child, parents) -> float:
        return self.family(child, parents)[0]


# ---- the score and the scan ----------------------------------------------------------------------

def family_params(k, child, parents) -> int:
    return (int(k[child]) - 1) * math.prod(int(k[u]) for u in parents)


def penalty_factor(criterion, total) -> float:
    return 1.0 if criterion == "aic" else math.log2(float(total)) / 2


def score_arith(ll, params, criterion, total) -> float:
    """evaluation.py's arithmetic on per-node sums: likelihood = 0.0; likelihood -= ll[v] in node order; + the penalty."""
    likelihood = 0.0
    for x in ll:
        likelihood -= float(x)
    if criterion == "aic":
        return likelihood + float(params)
    return likelihood + float(params) * (math.log2(float(total)) / 2)


def reaches(parents, a) -> set:
    """Every node with a path from `a` (a itself included): graph.hpp is_able_trace(a, .)."""
    children = [[] for _ in parents]
    for v, ps in enumerate(parents):
        for u in ps:
            children[u].append(v)
    seen, stack = {a}, [a]
    while stack:
        for c in children[stack.pop()]:
            if c not in seen:
                seen.add(c)
                stack.append(c)
    return seen


class RefLearner:
    """The reference's loop, one candidate at a time, over family terms from `ll_fn(child, parents)`.  `decisions` records
    per evaluated candidate (child, candidate, score_now, score_next, accepted, parents per node before the decision)."""

    def __init__(self, k, parents, criterion, total, ll_fn, max_parents=MAX_PARENTS, record=False):
        self.k, self.criterion, self.total, self.ll_fn, self.max_parents = [int(x) for x in k], criterion, int(total), ll_fn, max_parents
        self.n = len(self.k)
        self.parents = [sorted(int(u) for u in p) for p in parents]
        self.ll = [ll_fn(v, self.parents[v]) for v in range(self.n)]
        self.params = sum(family_params(self.k, v, self.parents[v]) for v in range(self.n))
        self.score = score_arith(self.ll, self.params, criterion, total)
        self.record, self.decisions = record, []

    def try_parents(self, child, cand):
        out = []
        for u in cand:
            u = int(u)
            par = self.parents[child]
            ok = u != child and u not in par and u not in reaches(self.parents, child)   # (graph.hpp:270: add_edge fails)
            ok = ok and len(par) + 1 <= min(self.max_parents, MAX_PARENTS)
            ok = ok and self.k[child] * self.k[u] * math.prod(self.k[x] for x in par) <= MAX_ENTRIES
            if not ok:
                out.append(False)
                continue
            nxt = sorted(par + [u])
            ll_next = self.ll_fn(child, nxt)
            params_next = self.params - family_params(self.k, child, par) + family_params(self.k, child, nxt)
            score_next = score_arith([ll_next if v == child else self.ll[v] for v in range(self.n)], params_next, self.criterion, self.total)
            take = score_next < self.score   # strict (greedy.hpp:47, k2_algorithm.hpp:54)
            if self.record:
                self.decisions.append((child, u, self.score, score_next, take, [list(p) for p in self.parents]))
            if take:
                self.parents[child], self.ll[child], self.params, self.score = nxt, ll_next, params_next, score_next
            out.append(take)
        return out


def run_greedy(L, orders):
    """greedy::operator() over given orders: (children, tails)."""
    flags = []
    for child, tail in zip(*orders):
        flags.append(L.try_parents(int(child), tail))
    return flags


run_hint = run_greedy   # learn_with_hint: (children, the parent candidates per child)


def run_k2(L, children, precondition=None):
    """k2_algorithm::operator(): candidates in node order but the target and precondition[target]; an accepted parent gets
    the target into ITS exclusion list (k2_algorithm.hpp:57)."""
    pre = {int(v): [int(x) for x in xs] for v, xs in (precondition or {}).items()}
    flags = []
    for target in children:
        target = int(target)
        cand = [v for v in range(L.n) if v != target and v not in pre.get(target, ())]
        got = L.try_parents(target, cand)
        for u, ok in zip(cand, got):
            if ok:
                pre.setdefault(u, []).append(target)
        flags.append((cand, list(got)))
    return flags


def greedy_orders(nodes, seed):
    """Child order and tails as the tests fix them: children permuted with default_rng(seed + 1), the tail of child i (the
    children after it) with default_rng(seed + 2 + i)."""
    nodes = [int(v) for v in nodes]
    children = [nodes[i] for i in np.random.default_rng(seed + 1).permutation(len(nodes))]
    tails = []
    for i in range(len(children)):
        tail = children[i + 1:]
        tails.append([tail[j] for j in np.random.default_rng(seed + 2 + i).permutation(len(tail))])
    return children, tails


# ---- margins and bounds (contracts 4 and 5) -------------------------------------------------------

def graph_bound(table: Table, parents, criterion) -> float:
    """B(G) = (8u + gamma_{M+n+2}) * (sum |t| + |p|): bounds |learner score - the score AIC / MDL give for G with fitted CPTs|."""
    mags, M = 0.0, 0
    for v, ps in enumerate(parents):
        _, mag, m = table.family(v, ps)
        mags += mag
        M += m
    params = sum(family_params(table.k, v, ps) for v, ps in enumerate(parents))
    p = float(params) * penalty_factor(criterion, table.total)
    return (8 * U + gamma(M + table.n + 2)) * (mags + abs(p))


def reference_bound(table: Table, parents, criterion, vertexes=None) -> float:
    """B_ref(G) = (8u + gamma_{M+n+2} + gamma_{M+2}) * (sum |t| + |p|): bounds |a score of this project (the learner's, or
    score_arith over libm terms) - what the reference's aic / mdl return for G with the CPTs its make_cpt fits|.

    graph_bound's gamma_{M+n+2} covers ONE computation whose terms each pass through at most M + n + 2 roundings (a family's
    partial sums and folds, the n subtractions in node order, the penalty's product and addition); it compares two
    computations only where the other side adds in the same stated order (AIC / MDL of evaluation.py do).  The reference
    (basic_info_criteria.hpp:51-89) keeps ONE running sum over all M non-zero terms of all nodes, in the iteration order of
    an unordered_map: an arbitrary order in which a term can pass through M - 1 additions, then the penalty's product and
    its addition, so its own distance to the exact sum of the same terms is at most gamma_{M+2} * (sum |t| + |p|), whatever
    the order.  The two errors add; 8u is graph_bound's allowance for the terms themselves (logarithm and product on either
    side).  `vertexes`: the likelihood runs over these nodes only (eval_(graph, vertex_list)); the penalty is always the
    whole graph's."""
    mags, M = 0.0, 0
    for v in (range(table.n) if vertexes is None else vertexes):
        _, mag, m = table.family(int(v), parents[int(v)])
        mags += mag
        M += m
    params = sum(family_params(table.k, v, ps) for v, ps in enumerate(parents))
    p = float(params) * penalty_factor(criterion, table.total)
    return (8 * U + gamma(M + table.n + 2) + gamma(M + 2)) * (mags + abs(p))


def margins(table: Table, L: RefLearner):
    """Per recorded decision of the public-API loop: (|score_next - score_now|, B(next) + B(now))."""
    out = []
    for child, u, now, nxt, _, parents in L.decisions:
        after = [list(p) for p in parents]
        after[child] = sorted(after[child] + [u])
        out.append((abs(nxt - now), graph_bound(table, after, L.criterion) + graph_bound(table, parents, L.criterion)))
    return out


# ---- the inputs the CPU test checks and the GPU test relies on ------------------------------------

def sample_table(model, draws, seed) -> Table:
    """`draws` forward samples (exact_refs.forward_sample, default_rng(seed)), equal rows merged in order of first appearance.
    forward_sample walks the nodes in id order, so in a network whose ids are not topological (the ALARM-shaped one) a parent with
    a larger id is read at state 0: still a table with strong dependencies, which is all the learners need."""
    from exact_refs import forward_sample
    rng = np.random.default_rng(seed)
    seen = {}
    for _ in range(draws):
        key = tuple(int(x) for x in forward_sample(model, rng))
        seen[key] = seen.get(key, 0) + 1
    return Table(np.array(list(seen.keys()), dtype=np.uint8), np.array(list(seen.values()), dtype=np.uint64), model.k)


_INPUTS = {}
INPUT_NAMES = ("alarm2k_aic", "alarm2k_mdl", "alarm20k_mdl", "dag60_mdl")


def learning_input(name):
    """(model, Table, criterion, (children, tails), max_parents) of one row of the issue's table; cached per process."""
    from bayesiannetwork_amd import synth
    from bayesiannetwork_amd.dsc import load_dsc
    spec = {"alarm2k_aic": ("alarm", 2000, 21, "aic"), "alarm2k_mdl": ("alarm", 2000, 21, "mdl"),
            "alarm20k_mdl": ("alarm", 20000, 5, "mdl"), "dag60_mdl": ("dag60", 5000, 9, "mdl")}[name]
    net, draws, seed, criterion = spec
    key = (net, draws, seed)
    if key not in _INPUTS:
        if net == "alarm":
            model, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
        else:
            model = synth.random_dag(60, 3, 16, 3, seed=4)
        _INPUTS[key] = (model, sample_table(model, draws, seed))
    model, table = _INPUTS[key]
    return model, table, criterion, greedy_orders(range(model.n), seed), 6


def hint_orders(n, seed):
    """learn_with_hint's orders for the tests: the first 20 nodes may become parents of the others; children permuted with
    default_rng(seed), the parents per child with default_rng(seed + 1 + i)."""
    parents, children = list(range(min(20, n))), list(range(min(20, n), n))
    children = [children[i] for i in np.random.default_rng(seed).permutation(len(children))]
    return children, [[parents[j] for j in np.random.default_rng(seed + 1 + i).permutation(len(parents))] for i in range(len(children))]


def k2_children(n, seed):
    return [int(v) for v in np.random.default_rng(seed).permutation(n)]


K2_PRECONDITION = {3: [0, 1, 2], 10: [4], 36: list(range(20))}


def empty_graph(n):
    return [[] for _ in range(n)]
