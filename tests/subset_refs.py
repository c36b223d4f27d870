"""Plain Python restatement of the exhaustive searches of include/bn_mi355x.h (bn_learn_best_parents, bn_learn_brute_force_hint,
bn_learn_brute_force) and a LITERAL transcription of the reference's recursions (bayesian/learning/brute_force.hpp), both over
family terms from `ll_fn(child, parents)` as tests/learning_refs.py has them: with `Table.libm_ll` they are the loop over the
public API (fit_cpt -> Engine -> AIC / MDL per enumerated graph) restated on the CPU, with the device's own terms they are what
the library must do bit for bit.  Also the subset lattice's index arithmetic (`sum_out`, `lattice_counts`)."""
import math

import numpy as np

import learning_refs as LR


# ---- the lattice: a family's counts from the top family's ------------------------------------------

def sum_out(N, outer, kx, inner):
    """out[h * inner + l] = sum over s < kx of N[(h * kx + s) * inner + l] -- one step of either kernel form."""
    return np.asarray(N, dtype=np.uint64).reshape(outer, kx, inner).sum(axis=1, dtype=np.uint64).reshape(-1)


def lattice_counts(top, k, child, base, cand):
    """Every family base + {cand[j] : bit j of mask} in the fitted layout, from the top family's counts: the absent candidates
    summed out one after another, smallest id first (the order of both kernel forms)."""
    ids = sorted([int(x) for x in base] + [int(x) for x in cand])
    out = []
    for mask in range(1 << len(cand)):
        N, dims = np.asarray(top, dtype=np.uint64), [int(k[u]) for u in ids] + [int(k[child])]
        keep = [u for u in ids if u in base or (mask >> list(cand).index(u)) & 1]
        pos = 0
        for u in ids:
            if u in keep:
                pos += 1
                continue
            N = sum_out(N, math.prod(dims[:pos]), dims[pos], math.prod(dims[pos + 1:]))
            del dims[pos]
        out.append(N)
    return out


def visiting_order(m):
    """The masks (bit j: cand[j]) in the order brute_force.hpp:104-111 meets them: "not added" before "added", cand[0] outermost."""
    return [sum(1 << j for j in range(m) if (r >> (m - 1 - j)) & 1) for r in range(1 << m)]


# ---- the restatement of the library's searches -------------------------------------------------------

class RefSearch(LR.RefLearner):
    """RefLearner plus the exhaustive searches, decided as include/bn_mi355x.h states them."""

    def _score(self, parents, vertexes=None):
        ll = [self.ll_fn(v, parents[v]) for v in (range(self.n) if vertexes is None else vertexes)]
        params = sum(LR.family_params(self.k, v, parents[v]) for v in range(self.n))
        return LR.score_arith(ll, params, self.criterion, self.total)

    def _room(self, child):
        return min(self.max_parents, LR.MAX_PARENTS) - len(self.parents[child])

    def _set(self, parents):
        self.parents = [sorted(p) for p in parents]
        self.ll = [self.ll_fn(v, self.parents[v]) for v in range(self.n)]
        self.params = sum(LR.family_params(self.k, v, self.parents[v]) for v in range(self.n))
        self.score = LR.score_arith(self.ll, self.params, self.criterion, self.total)

    def survivors(self, child, cand):
        par, reach, room = self.parents[child], LR.reaches(self.parents, child), self._room(child)
        surv, at = [], []
        for i, u in enumerate(int(x) for x in cand):
            if room <= 0 or u in reach or u in par or u in surv:
                continue
            if self.k[child] * self.k[u] * math.prod(self.k[x] for x in par) > LR.MAX_ENTRIES:
                continue
            surv.append(u)
            at.append(i)
        return surv, at

    def subset_scores(self, child, surv):
        """{mask: score of the graph with the subset added}, eligible subsets only, in visiting order."""
        out = {}
        for mask in visiting_order(len(surv)):
            S = [surv[j] for j in range(len(surv)) if (mask >> j) & 1]
            if len(S) > self._room(child):
                continue
            nxt = sorted(self.parents[child] + S)
            params = self.params - LR.family_params(self.k, child, self.parents[child]) + LR.family_params(self.k, child, nxt)
            out[mask] = LR.score_arith([self.ll_fn(child, nxt) if v == child else self.ll[v] for v in range(self.n)], params, self.criterion,
                                       self.total)
        return out

    def best_parents(self, child, cand):
        taken = [False] * len(cand)
        surv, at = self.survivors(child, cand)
        if not surv:
            return taken
        best_mask, best = 0, None
        for mask, score in self.subset_scores(child, surv).items():   # (insertion order: the visiting order)
            if best is None or score < best:
                best_mask, best = mask, score
        if best_mask == 0:
            return taken
        S = [surv[j] for j in range(len(surv)) if (best_mask >> j) & 1]
        nxt = sorted(self.parents[child] + S)
        self.params += LR.family_params(self.k, child, nxt) - LR.family_params(self.k, child, self.parents[child])
        self.parents[child], self.ll[child], self.score = nxt, self.ll_fn(child, nxt), best
        for j in range(len(surv)):
            if (best_mask >> j) & 1:
                taken[at[j]] = True
        return taken

    def decomposes(self, par, child):
        return not any(set(LR.reaches(self.parents, int(c))) & {int(p) for p in par} for c in child)

    def brute_force_hint(self, par, child):
        par, child = [int(x) for x in par], [int(x) for x in child]
        if self.decomposes(par, child):
            done = set()
            for c in child:
                if c not in done:
                    done.add(c)
                    self.best_parents(c, par)
            return self.score
        if len(par) * len(child) > 20:
            raise ValueError("more than 20 possible edges")
        best, score, _ = literal_hint(self, par, child)
        self._set(best)
        assert self.score == score
        return self.score

    def brute_force(self, vertexes):
        """The enumeration with the repeated "no edge" branches left out; returns the reference's evaluated quantity."""
        vs = [int(v) for v in vertexes]
        assert len(vs) <= 8 and len(set(vs)) == len(vs)
        g = Graph(self.parents, min(self.max_parents, LR.MAX_PARENTS))
        state = {"graph": [list(p) for p in self.parents], "eval": self._score(self.parents, vs)}

        def rec(t):
            if t == len(vs) - 1:
                now = self._score(g.parents, vs)
                if now < state["eval"]:
                    state["eval"], state["graph"] = now, [sorted(p) for p in g.parents]
                return
            for i in range(t + 1, len(vs)):
                if i == t + 1:
                    rec(t + 1)
                for a, b in ((vs[t], vs[i]), (vs[i], vs[t])):
                    if g.add_edge(a, b):
                        rec(t + 1)
                        g.erase_edge(a, b)
        if vs:
            rec(0)
        self._set(state["graph"])
        return state["eval"]


# ---- the reference's recursions, literally -------------------------------------------------------------

class Graph:
    """graph_t as the recursions use it: add_edge refuses an existing edge and one that closes a cycle (graph.hpp:268-275), and --
    the library's limit -- one beyond max_parents."""

    def __init__(self, parents, max_parents=LR.MAX_PARENTS):
        self.parents, self.max_parents = [list(p) for p in parents], max_parents

    def add_edge(self, u, c):
        if u == c or u in self.parents[c] or u in LR.reaches(self.parents, c) or len(self.parents[c]) >= self.max_parents:
            return False
        self.parents[c].append(u)
        return True

    def erase_edge(self, u, c):
        self.parents[c].remove(u)


def literal_hint(L: RefSearch, par, child):
    """brute_force.hpp:51-113.  Returns (best parents per node, best score, [(parents per node, score) per evaluated leaf])."""
    edges = [(int(p), int(c)) for p in par for c in child]   # (:61-67)
    g = Graph(L.parents, min(L.max_parents, LR.MAX_PARENTS))
    state = {"graph": [sorted(p) for p in L.parents], "eval": L._score(L.parents)}
    leaves = []

    def rec(e):
        if e == len(edges):
            now = L._score(g.parents)
            leaves.append(([sorted(p) for p in g.parents], now))
            if now < state["eval"]:
                state["eval"], state["graph"] = now, [sorted(p) for p in g.parents]
            return
        rec(e + 1)
        if g.add_edge(*edges[e]):
            rec(e + 1)
            g.erase_edge(*edges[e])
    rec(0)
    return state["graph"], state["eval"], leaves


def literal_brute_force(L: RefSearch, vertexes):
    """brute_force.hpp:32-44, :116-156.  Returns (best parents per node, best eval_(graph, vertexes), the evaluated leaves)."""
    vs = [int(v) for v in vertexes]
    g = Graph(L.parents, min(L.max_parents, LR.MAX_PARENTS))
    state = {"graph": [sorted(p) for p in L.parents], "eval": L._score(L.parents, vs)}
    leaves = []

    def rec(t):
        if t == len(vs) - 1:
            now = L._score(g.parents, vs)
            leaves.append(([sorted(p) for p in g.parents], now))
            if now < state["eval"]:
                state["eval"], state["graph"] = now, [sorted(p) for p in g.parents]
            return
        for i in range(t + 1, len(vs)):
            rec(t + 1)
            if g.add_edge(vs[t], vs[i]):
                rec(t + 1)
                g.erase_edge(vs[t], vs[i])
            if g.add_edge(vs[i], vs[t]):
                rec(t + 1)
                g.erase_edge(vs[i], vs[t])
    if vs:
        rec(0)
    return state["graph"], state["eval"], leaves


# ---- the inputs the CPU test checks and the GPU test relies on ------------------------------------------

HINT_CHILDREN, HINT_CANDIDATES = 10, 5


def hint_calls(name):
    """The hint searches of one of learning_refs' inputs: HINT_CHILDREN children drawn with default_rng(77); per child one
    learn_with_hint(parents, [child]) whose parent set is the child's neighbours in the generating network (its parents, then its
    children, at most 3) filled to HINT_CANDIDATES with distractors drawn from the other nodes.  Made one after another on one
    learner that starts with no edges."""
    model, table, criterion, _, max_parents = LR.learning_input(name)
    rng = np.random.default_rng(77)
    children = [int(c) for c in rng.permutation(model.n)[:HINT_CHILDREN]]
    calls = []
    for c in children:
        near = [int(u) for u in model.parents(c)] + [v for v in range(model.n) if c in model.parents(v).tolist()]
        par = near[:3]
        for u in rng.permutation(model.n):
            if len(par) >= HINT_CANDIDATES:
                break
            if int(u) != c and int(u) not in par:
                par.append(int(u))
        calls.append(([par[i] for i in rng.permutation(len(par))], [c]))
    return model, table, criterion, max_parents, calls


def neighbourhood(model, calls, size):
    """`size` vertexes for brute_force: the first child of `calls` with at least two neighbours in the generating network, its
    neighbours, then the nodes in id order."""
    def near(c):
        return [int(u) for u in model.parents(c)] + [v for v in range(model.n) if c in model.parents(v).tolist()]
    c = next(c for _, (c,) in calls if len(near(c)) >= 2)
    return ([c] + near(c) + [v for v in range(model.n) if v not in near(c) and v != c])[:size]
