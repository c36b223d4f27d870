"""Plain Python restatement of the hill-climbing contract of include/bn_mi355x.h (bn_learn_climb): steepest descent over add,
delete and reverse moves with a tabu list over node pairs and perturbed restarts.

It works over term ROWS: rows[c][r] is the family term of child c at index r of the term table (anneal_refs.rank).  The graph is
held as parent LISTS, reachability is a depth-first walk over child lists made from them (no ancestor or descendant masks, which
is what the kernel keeps), a reversal's second path is looked for on the graph with the edge taken out.  `climb_run` is one run;
`literal_moves` is a second routine that lists the legal moves of a graph by trying each one and sorting the result
topologically."""
import math
import struct

import anneal_refs as AR
import learning_refs as LR

END_NO_MOVE, END_OPTIMUM, END_CAP = 1, 2, 4
KINDS = ("add", "delete", "reverse")


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


class LazyRows:
    """rows[c][r] over a term function: the entry is made when it is asked for (anneal_refs.unrank gives the parent set)."""

    class _Row:
        def __init__(self, n, q, c, term):
            self.n, self.q, self.c, self.term, self.have = n, q, c, term, {}

        def __getitem__(self, r):
            if r not in self.have:
                self.have[r] = float(self.term(self.c, tuple(AR.unrank(self.n, self.q, self.c, r))))
            return self.have[r]

    def __init__(self, n, q, term):
        self.rows = [LazyRows._Row(n, q, c, term) for c in range(n)]

    def __getitem__(self, c):
        return self.rows[c]


class Problem:
    """What a run climbs over: arities, the in-degree bound mp, the criterion ("aic", "mdl", or "bdeu": the likelihood alone), the
    table's total count (MDL's penalty), the term rows and the starting parent lists.  `prefetch`, where set, is called with the
    parent lists before every look at the moves (scripts/time_climb.py fills its rows through it)."""
    prefetch = None

    def __init__(self, k, mp, criterion, total, rows, start=None):
        self.k, self.n, self.mp, self.criterion, self.total, self.rows = [int(x) for x in k], len(k), int(mp), criterion, int(total), rows
        self.start = [sorted(p) for p in start] if start is not None else [[] for _ in k]
        self.penalty = LR.penalty_factor(criterion, total) if criterion in ("aic", "mdl") else 0.0
        self._deltas = {}

    def term(self, c, parents):
        return float(self.rows[c][AR.rank(self.n, c, parents)])

    def rows_of(self, parents):
        return math.prod(self.k[u] for u in parents)

    def score(self, ll, params):
        if self.criterion in ("aic", "mdl"):
            return LR.score_arith(ll, params, self.criterion, self.total)
        likelihood = 0.0
        for x in ll:
            likelihood -= float(x)
        return likelihood

    def delta(self, c, ll_c, old, new):
        """Of child c's family going from parent list `old` (whose term is ll_c) to `new`: (term_new, d)."""
        key = (c, tuple(old), tuple(new))
        if key not in self._deltas:
            self._deltas[key] = self._delta(c, ll_c, old, new)
        return self._deltas[key]

    def _delta(self, c, ll_c, old, new):
        t = self.term(c, new)
        d = ll_c - t
        dp = (self.k[c] - 1) * self.rows_of(new) - (self.k[c] - 1) * self.rows_of(old)
        if self.criterion == "aic":
            d = d + float(dp)
        elif self.criterion == "mdl":
            d = d + float(dp) * self.penalty
        return t, d


def children_of(parents):
    ch = [[] for _ in parents]
    for v, ps in enumerate(parents):
        for u in ps:
            ch[u].append(v)
    return ch


def walk(children, a):
    """Every node a path leads to from `a`, `a` itself not included unless it lies on a cycle: a depth-first walk."""
    seen, stack = set(), [a]
    while stack:
        for c in children[stack.pop()]:
            if c not in seen:
                seen.add(c)
                stack.append(c)
    return seen


def moves_of(pb, parents, ll, events=None):
    """{id: d} of every legal move of the graph, looked at as the contract words it."""
    def note(name):
        if events is not None:
            events[name] = events.get(name, 0) + 1

    n = pb.n
    ch = children_of(parents)
    below = [walk(ch, v) for v in range(n)]   # what v reaches
    out = {}
    for frm in range(n):
        for to in range(n):
            if frm == to:
                continue
            if frm not in parents[to]:
                if frm in below[to]:
                    note("refused_cycle")
                    continue
                if len(parents[to]) >= pb.mp:
                    note("refused_mp")
                    continue
                t, d = pb.delta(to, ll[to], parents[to], sorted(parents[to] + [frm]))
                if t != t or d != d:
                    note("refused_nan")
                    continue
                out[(0 * n + frm) * n + to] = d
            else:
                less = [u for u in parents[to] if u != frm]
                _, d1 = pb.delta(to, ll[to], parents[to], less)
                if d1 == d1:
                    out[(1 * n + frm) * n + to] = d1
                without = [list(p) for p in parents]
                without[to] = less
                if to in walk(children_of(without), frm):
                    note("refused_second_path")
                    continue
                if len(parents[frm]) >= pb.mp:
                    note("refused_mp")
                    continue
                t2, d2 = pb.delta(frm, ll[frm], parents[frm], sorted(parents[frm] + [to]))
                d = d1 + d2
                if t2 != t2 or d != d:
                    note("refused_nan")
                    continue
                out[(2 * n + frm) * n + to] = d
    return out


def is_dag(parents):
    """Kahn's sort: every node leaves the queue iff the graph has no cycle."""
    n = len(parents)
    indeg = [len(p) for p in parents]
    ch = children_of(parents)
    queue = [v for v in range(n) if indeg[v] == 0]
    done = 0
    while queue:
        v = queue.pop()
        done += 1
        for c in ch[v]:
            indeg[c] -= 1
            if indeg[c] == 0:
                queue.append(c)
    return done == n


def applied(parents, kind, frm, to):
    new = [list(p) for p in parents]
    if kind == 0:
        new[to] = sorted(new[to] + [frm])
    else:
        new[to].remove(frm)
        if kind == 2:
            new[frm] = sorted(new[frm] + [to])
    return new


def literal_moves(pb, parents, ll):
    """{id: d} again, the literal way: make the move, then ask whether the result is a DAG within the bound with terms that are
    numbers; d from the terms of the two graphs."""
    n = pb.n
    out = {}
    for kind in range(3):
        for frm in range(n):
            for to in range(n):
                if frm == to or (frm in parents[to]) != (kind != 0):
                    continue
                new = applied(parents, kind, frm, to)
                if not is_dag(new) or (kind == 0 and len(new[to]) > pb.mp) or (kind == 2 and len(new[frm]) > pb.mp):
                    continue
                t, d = pb.delta(to, ll[to], parents[to], new[to])
                if t != t:
                    continue
                if kind == 2:
                    t2, d2 = pb.delta(frm, ll[frm], parents[frm], new[frm])
                    if t2 != t2:
                        continue
                    d = d + d2
                if d == d:
                    out[(kind * n + frm) * n + to] = d
    return out


def pick(moves, tabu, n):
    """The contract's choice among {id: d}: strictly smallest d by <, the lowest id among equals; tabu: a set of frozenset pairs.
    Returns (id or None, d, legal-but-tabu count, ties: the moves that share the smallest d)."""
    best, best_d, tabu_legal, ties = None, 0.0, 0, 0
    for mid in sorted(moves):
        d = moves[mid]
        if frozenset(((mid // n) % n, mid % n)) in tabu:
            tabu_legal += 1
            continue
        if best is None or d < best_d:
            best, best_d, ties = mid, d, 1
        elif d == best_d:
            ties += 1
    return best, best_d, tabu_legal, ties


def climb_run(pb, tabu_len, max_worse, max_steps, perturb, seed, j, events=None):
    """Run j.  Returns score (best_eval), the six counts, masks of the best graph, its ll and parameter count, the trace (kind,
    from, to, bits of d, bits of current), the score of the graph the climb started from, and `graphs`: the parent lists after
    every applied step."""
    def note(name):
        if events is not None:
            events[name] = events.get(name, 0) + 1

    n, k = pb.n, pb.k
    max_steps = max_steps or (1 << 16)
    parents = [list(p) for p in pb.start]
    ll = [pb.term(v, parents[v]) for v in range(n)]

    def apply(kind, frm, to):
        nonlocal parents
        parents = applied(parents, kind, frm, to)
        for c in (to, frm) if kind == 2 else (to,):
            ll[c] = pb.term(c, parents[c])

    def evaluate():
        return pb.score(ll, sum((k[v] - 1) * pb.rows_of(parents[v]) for v in range(n)))

    perturbed = 0
    if j >= 1 and perturb > 0:
        rng = AR.Stream(seed, j)
        for _ in range(perturb):
            kind, frm, to = rng.below(3), rng.below(n), rng.below(n)
            if (kind * n + frm) * n + to in moves_of(pb, parents, ll) and frm != to:
                apply(kind, frm, to)
                perturbed += 1
    current = start_score = evaluate()
    best_eval, best = current, ([list(p) for p in parents], list(ll))
    steps = improving = best_step = worse = flags = tabu_legal = 0
    ring, trace, graphs = [], [], []
    while steps < max_steps:
        if pb.prefetch is not None:
            pb.prefetch(parents)
        moves = moves_of(pb, parents, ll, events)
        tabu = set(ring[-tabu_len:]) if tabu_len > 0 else set()
        mid, d, tabu_legal, ties = pick(moves, tabu, n)
        if mid is None:
            flags = END_NO_MOVE
            break
        if not d < 0 and worse == max_worse:
            flags = END_OPTIMUM
            break
        if ties > 1:
            note("tie_by_id")
        if tabu and pick(moves, set(), n)[0] != mid:
            note("tabu_changed_choice")
        kind, frm, to = mid // (n * n), (mid // n) % n, mid % n
        apply(kind, frm, to)
        steps += 1
        improving += d < 0
        ring.append(frozenset((frm, to)))
        current = evaluate()
        trace.append((kind, frm, to, bits(d), bits(current)))
        graphs.append([list(p) for p in parents])
        note(KINDS[kind] + "_applied")
        if current < best_eval:
            best_eval, best, best_step, worse = current, ([list(p) for p in parents], list(ll)), steps, 0
        else:
            worse += 1
    if flags == 0:
        flags = END_CAP
    bp, bll = best
    return {"score": best_eval, "steps": steps, "improving": improving, "perturbed": perturbed, "best_step": best_step, "flags": flags,
            "tabu_legal": tabu_legal, "masks": [sum(1 << u for u in p) for p in bp], "parents": bp, "ll": bll,
            "params": sum((k[v] - 1) * pb.rows_of(bp[v]) for v in range(n)), "trace": trace, "start_score": start_score,
            "graphs": graphs, "final_parents": parents, "final_ll": list(ll)}


# ---- the fixed inputs of the CPU and the GPU tests --------------------------------------------------

_TIES = []


def ties_input():
    """anneal_refs' n6 (arities 2, 1, 3, 4, 2, 5) with column 4 made a copy of column 0: the families that differ only in which
    of the two is a parent have the same counts, hence terms and deltas with the same bits."""
    if not _TIES:
        model, table = AR.anneal_input("n6")
        pats = table.pats.copy()
        pats[:, 4] = pats[:, 0]
        _TIES.append((model, LR.Table(pats, table.counts, table.k)))
    return _TIES[0]


def climb_input(name):
    return ties_input() if name == "ties6" else AR.anneal_input(name)


# the edges of the n33 input's generating model turned round, at most three parents kept per node
REVERSED33 = [[2, 3, 6], [4, 10], [4, 9, 14], [], [7, 14], [9, 15, 20], [13], [], [13, 16, 19], [], [19, 25], [], [], [], [17], [20, 29],
              [25, 26], [19, 24, 25], [21, 28], [20, 26, 30], [30], [29], [26, 27], [28], [], [], [30], [29], [], [], [], [], []]

# name: (input, table q, criterion, mp, tabu_len, max_worse, max_steps, perturb, runs, seed, start)
# mp: the in-degree bound handed to the call (below the table's q where a row says so)
RUNS = {
    "n6_greedy_aic": ("n6", 3, "aic", 3, 0, 0, 0, 0, 1, 1, None),
    "n6_tabu_mdl": ("n6", 3, "mdl", 3, 4, 6, 0, 3, 5, 2, None),
    "ties6_greedy": ("ties6", 3, "aic", 3, 0, 0, 0, 0, 1, 3, None),                 # equal d: the lowest id
    "ties6_tabu_bdeu": ("ties6", 3, "bdeu", 3, 3, 5, 40, 4, 4, 4, None),
    "n6_second_path": ("n6", 3, "mdl", 3, 2, 4, 0, 0, 1, 5, [[], [], [0], [0, 2], [], []]),   # 0 -> 2 -> 3 and 0 -> 3
    "n2_no_move": ("n2", 1, "aic", 1, 1, 5, 0, 0, 1, 6, None),                   # one pair, tabu after the first step: flag 1
    "bigk_nan": ("bigk", 3, "aic", 3, 2, 3, 20, 2, 3, 7, [[1], [], [], [0, 1]]),    # 255^3 entries: terms that are NaN
    "n33_greedy_mdl": ("n33", 3, "mdl", 3, 0, 0, 0, 0, 1, 8, None),
    "n33_reversed_mdl": ("n33", 3, "mdl", 3, 0, 0, 0, 0, 1, 15, REVERSED33),         # reversals are the improving moves
    "n33_tabu_aic_mp2": ("n33", 3, "aic", 2, 8, 6, 30, 6, 3, 9, None),              # mp below the table's q
    "n33_dense_bdeu": ("n33", 3, "bdeu", 3, 5, 4, 12, 5, 3, 10, AR.DENSE33),        # dense at mp parents
    "n64_path_cap": ("n64", 2, "aic", 2, 0, 0, 6, 0, 1, 11, AR.PATH64),             # ends at max_steps: flag 4
    "n64_path_tabu_mdl": ("n64", 2, "mdl", 2, 64, 3, 10, 8, 3, 12, AR.PATH64),
    "n64_empty_greedy": ("n64", 2, "aic", 2, 0, 0, 12, 0, 1, 13, None),
    "n64_dense_mp1": ("n64", 2, "mdl", 1, 3, 2, 8, 4, 2, 14, AR.dense_start(64, 1)),
}
WAVES = 4   # runs per workgroup (bn_learn_climb.hpp): 4 * WAVES + 1 runs fill four workgroups and start a fifth


def cpu_term(name):
    """The libm term function of a row's input and criterion."""
    inp, q, criterion = RUNS[name][:3]
    _, table = climb_input(inp)
    if criterion == "bdeu":
        import bd_refs as BD
        return BD.bd_term_fn(BD.BDTable(table, BD.BDEU1))
    return AR.libm_term(table)


def run_setup(name, rows=None):
    """(Problem, keyword arguments of climb_run but j, runs) of one row of RUNS; rows: the term rows (default: libm, made lazily)."""
    inp, q, criterion, mp, tabu_len, max_worse, max_steps, perturb, runs, seed, start = RUNS[name]
    _, table = climb_input(inp)
    if rows is None:
        rows = LazyRows(table.n, q, cpu_term(name))
    pb = Problem(table.k, min(mp, q), criterion, table.total, rows, start)
    return pb, dict(tabu_len=tabu_len, max_worse=max_worse, max_steps=max_steps, perturb=perturb, seed=seed), runs
