"""Plain Python restatement of the annealing contract of include/bn_mi355x.h (bn_terms_*, bn_learn_anneal) and a literal
transcription of the reference's loop (bayesian/learning/simulated_annealing.hpp:41-115 over graph.hpp's graph_t).

Index of the term table (restated from the header): relabel the nodes other than the child c to 0 .. n-2 by s' = s - (s > c); for
S = {s'_1 < ... < s'_j}: rank = offset[j] + sum_{i=1..j} C(s'_i, i), offset[j] = sum_{t<j} C(n-1, t); T(n, q) = offset[q+1].

`literal_chain` is the reference's code line for line on `RefGraph`, a small graph class with graph_t's edge_list semantics
(append on add, ordered erase, the re-append of a refused reversal, copy-back on rejection).  `restated_chain` is what the kernel
does: parent masks, an ordered list, the list of the last accepted graph, incremental parameter counts.  Both draw from the
library's stream: chain j owns xoshiro128++ seeded by Philox4x32-10({j_lo, j_hi, 0, 0}, {seed_lo, seed_hi})."""
import math
import struct
from math import comb

import numpy as np

import learning_refs as LR

M32 = 0xFFFFFFFF
END_TEMPERATURE, END_SAME_STATE, END_CAP = 1, 2, 4
MAX_ENTRIES = 1 << 20


# ---- the index -----------------------------------------------------------------------------------

def row_entries(n, q):
    return sum(comb(n - 1, t) for t in range(q + 1))


def rank(n, child, parents):
    ps = sorted(int(u) for u in parents)
    r = sum(comb(n - 1, t) for t in range(len(ps)))
    return r + sum(comb(u - (u > child), i + 1) for i, u in enumerate(ps))


def unrank(n, q, child, r):
    """The parent set at index r of the child's row (the inverse of `rank`)."""
    j = 0
    while r >= comb(n - 1, j):
        r -= comb(n - 1, j)
        j += 1
    assert j <= q
    out = []
    for i in range(j, 0, -1):   # the largest element first: the largest a with C(a, i) <= r
        a = i - 1
        while comb(a + 1, i) <= r:
            a += 1
        r -= comb(a, i)
        out.append(a + (a >= child))
    return sorted(out)


# ---- the stream ----------------------------------------------------------------------------------

def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def _rotl(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


class Stream:
    def __init__(self, seed, j):
        self.x = philox4x32_10((j & M32, (j >> 32) & M32, 0, 0), (seed & M32, (seed >> 32) & M32))
        if not any(self.x):
            self.x[0] = 1

    def next(self):
        x = self.x
        result = (_rotl((x[0] + x[3]) & M32, 7) + x[0]) & M32
        t = (x[1] << 9) & M32
        x[2] ^= x[0]
        x[3] ^= x[1]
        x[1] ^= x[2]
        x[0] ^= x[3]
        x[2] ^= t
        x[3] = _rotl(x[3], 11)
        return result

    def below(self, m):
        return (self.next() * m) >> 32

    def uniform(self):
        return (self.next() + 0.5) * 2.0 ** -32


# ---- the problem ---------------------------------------------------------------------------------

class Problem:
    """What a chain runs over: arities, the in-degree bound, the criterion and `term(child, sorted parent tuple)` (NaN: not
    eligible)."""

    def __init__(self, k, q, criterion, total, term, start=None):
        self.k, self.n, self.q, self.criterion, self.total, self.term = [int(x) for x in k], len(k), int(q), criterion, int(total), term
        self.start = [sorted(p) for p in start] if start is not None else [[] for _ in k]

    def score(self, ll, params):
        return LR.score_arith(ll, params, self.criterion, self.total)


class Schedule:
    def __init__(self, initial_temp, final_temp, rate, boltzmann=1.0, same_state_max=100, rule="reference", max_proposals=1 << 20):
        self.t0, self.t1, self.rate, self.boltzmann, self.same_state_max = initial_temp, final_temp, rate, boltzmann, same_state_max
        self.rule, self.max_proposals = rule, max_proposals


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _accept(sched, rng, now, current, temperature, uphill):
    diff = now - current
    if diff <= 0:
        return True
    u = rng.uniform()
    scale = sched.boltzmann * temperature
    p = math.exp(-(now if sched.rule == "reference" else diff) / scale)
    uphill.append((u, p))
    return u < p


def _flags(sched, temperature, no_changed, proposals):
    return ((0 if temperature > sched.t1 else END_TEMPERATURE) | (0 if no_changed < sched.same_state_max else END_SAME_STATE) |
            (0 if proposals < sched.max_proposals else END_CAP))


# ---- the literal transcription -------------------------------------------------------------------

class RefGraph:
    """graph_t with integer vertexes: edge_list_ (insertion order), adjacent_list_[from][to].  `eligible(to, parents)` is the
    library's addition to add_edge: the in-degree bound and the NaN terms."""

    def __init__(self, n, eligible):
        self.n, self.eligible = n, eligible
        self.edge_list = []
        self.adj = [[None] * n for _ in range(n)]

    def copy(self):
        g = RefGraph(self.n, self.eligible)
        g.edge_list = list(self.edge_list)
        g.adj = [row[:] for row in self.adj]
        return g

    def out_vertexes(self, v):
        return [j for j in range(self.n) if self.adj[v][j] is not None]

    def in_vertexes(self, v):
        return [i for i in range(self.n) if self.adj[i][v] is not None]

    def is_able_trace(self, a, b, dead=None):   # graph.hpp:437
        """The reference's depth-first walk.  It visits a node once per PATH that leads to it, which on the dense starting graphs
        is more than 2^40 visits; `dead` holds the nodes a walk has already left without finding b.  The graph does not change
        during a walk, so a second visit would fail as the first did: the same answer, in the same order, without the repeats."""
        if a == b:
            return True
        dead = set() if dead is None else dead
        for c in self.out_vertexes(a):
            if c not in dead and self.is_able_trace(c, b, dead):
                return True
        dead.add(a)
        return False

    def edge_search(self, e):
        for i in range(self.n):
            for j in range(self.n):
                if self.adj[i][j] is e:
                    return i, j
        return None

    def add_edge(self, frm, to):   # :268
        if self.is_able_trace(to, frm):
            return None
        if self.adj[frm][to] is not None:
            return None
        if not self.eligible(to, sorted(self.in_vertexes(to) + [frm])):
            return None
        e = object()
        self.edge_list.append(e)
        self.adj[frm][to] = e
        return e

    def erase_edge(self, e):   # :309
        at = self.edge_search(e)
        if at is None:
            return False
        self.edge_list = [x for x in self.edge_list if x is not e]
        self.adj[at[0]][at[1]] = None
        return True

    def change_edge_direction(self, e):   # :339
        frm, to = self.edge_search(e)
        if not self.erase_edge(e):
            return None
        new = self.add_edge(to, frm)
        if new is not None:
            return new
        self.add_edge(frm, to)
        return None

    def edges(self):
        return [self.edge_search(e) for e in self.edge_list]


def _eligible(pb):
    def ok(to, parents):
        if len(parents) > pb.q:
            return False
        x = pb.term(to, tuple(parents))
        return x == x
    return ok


def literal_chain(pb, sched, seed, j):
    rng = Stream(seed, j)
    graph = RefGraph(pb.n, _eligible(pb))
    for v in range(pb.n):          # the starting graph: child-major, parents increasing
        for u in pb.start[v]:
            e = object()
            graph.edge_list.append(e)
            graph.adj[u][v] = e

    def evaluate(g):   # sampling_.make_cpt(graph); eval_(graph)
        fam = [tuple(g.in_vertexes(v)) for v in range(pb.n)]
        return pb.score([pb.term(v, fam[v]) for v in range(pb.n)], sum(LR.family_params(pb.k, v, fam[v]) for v in range(pb.n)))

    best_graph = graph.copy()
    best_eval = evaluate(graph)
    no_changed_num, temperature = 0, sched.t0
    proposals = operated = accepted = 0
    trace, uphill = [], []
    while temperature > sched.t1 and no_changed_num < sched.same_state_max and proposals < sched.max_proposals:
        proposals += 1
        is_operated = False
        method = rng.below(3)
        if method == 0:
            frm = rng.below(pb.n)
            to = rng.below(pb.n)
            if graph.add_edge(frm, to) is not None:
                is_operated = True
        else:
            edges = graph.edge_list
            if len(edges) < 1:
                continue
            target_edge = edges[rng.below(len(edges))]
            frm, to = graph.edge_search(target_edge)
            if method == 1:
                if graph.erase_edge(target_edge):
                    is_operated = True
            elif graph.change_edge_direction(target_edge) is not None:
                is_operated = True
        if not is_operated:
            continue
        operated += 1
        now_eval = evaluate(graph)
        is_acceptance = _accept(sched, rng, now_eval, best_eval, temperature, uphill)
        trace.append((method, frm, to, bits(now_eval), is_acceptance))
        if is_acceptance:
            best_graph = graph.copy()
            best_eval = now_eval
            no_changed_num = 0
            accepted += 1
        else:
            graph = best_graph.copy()
            no_changed_num += 1
        temperature *= sched.rate
    masks = [sum(1 << u for u in graph.in_vertexes(v)) for v in range(pb.n)]
    return {"eval": best_eval, "proposals": proposals, "operated": operated, "accepted": accepted,
            "flags": _flags(sched, temperature, no_changed_num, proposals), "masks": masks, "edges": graph.edges(), "trace": trace,
            "uphill": uphill}


# ---- what the kernel does ------------------------------------------------------------------------

def _parents_of(mask):
    return tuple(u for u in range(64) if (mask >> u) & 1)


def restated_chain(pb, sched, seed, j, events=None):
    """Masks, an ordered list, the list of the last accepted graph.  `events`: a dict that counts what happened."""
    def note(name):
        if events is not None:
            events[name] = events.get(name, 0) + 1

    n, k = pb.n, pb.k
    rng = Stream(seed, j)
    pm = [sum(1 << u for u in pb.start[v]) for v in range(n)]
    rows = [math.prod(k[u] for u in pb.start[v]) for v in range(n)]
    ll = [pb.term(v, tuple(pb.start[v])) for v in range(n)]
    lst = [(u, v) for v in range(n) for u in pb.start[v]]
    kept = list(lst)
    params = sum((k[v] - 1) * rows[v] for v in range(n))
    current, temperature = pb.score(ll, params), sched.t0
    no_changed = proposals = operated = accepted = 0
    trace, uphill = [], []
    longest = len(lst)

    def reaches(masks, a, b):
        if a == b:
            return True
        reached = frontier = 1 << a
        for _ in range(n):
            nxt = sum(1 << v for v in range(n) if masks[v] & frontier) & ~reached
            if (nxt >> b) & 1:
                return True
            if not nxt:
                return False
            reached |= nxt
            frontier = nxt
        return False

    while temperature > sched.t1 and no_changed < sched.same_state_max and proposals < sched.max_proposals:
        proposals += 1
        method = rng.below(3)
        new = {}   # node -> (mask, rows, ll) of the proposal
        if method == 0:
            frm, to = rng.below(n), rng.below(n)
            why = None
            if frm == to:
                why = "refused_self"
            elif reaches(pm, to, frm):
                why = "refused_cycle"
            elif (pm[to] >> frm) & 1:
                why = "refused_existing"
            elif bin(pm[to]).count("1") >= pb.q:
                why = "refused_q"
            else:
                mask = pm[to] | (1 << frm)
                x = pb.term(to, _parents_of(mask))
                if x != x:
                    why = "refused_nan"
                else:
                    new[to] = (mask, rows[to] * k[frm], x)
            if why:
                note(why)
                continue
            lst.append((frm, to))
        else:
            if not lst:
                note("no_edges")
                continue
            at = rng.below(len(lst))
            tail = len(lst) - 1 - at   # the entries the ordered erase moves down: the kernel moves 64 of them per round
            if tail > 64:
                note("erase_tail_gt64")
            if tail > 128:
                note("erase_tail_gt128")
            frm, to = lst.pop(at)
            without = list(pm)
            without[to] &= ~(1 << frm)
            ok = True
            if method == 2:
                ok = not reaches(without, frm, to) and bin(pm[frm]).count("1") < pb.q
                if ok:
                    mask = pm[frm] | (1 << to)
                    x = pb.term(frm, _parents_of(mask))
                    ok = x == x
                    if ok:
                        new[frm] = (mask, rows[frm] * k[to], x)
                if not ok:
                    lst.append((frm, to))   # added back at the END: the list stays reordered
                    note("reverse_refused")
                    if at != len(lst) - 1:
                        note("reverse_refused_moved")
                        if len(lst) > 64:
                            note("reverse_refused_moved_gt64")
                    continue
                lst.append((to, frm))
            new[to] = (without[to], rows[to] // k[frm], pb.term(to, _parents_of(without[to])))
        operated += 1
        longest = max(longest, len(lst))
        ll_new = [new[v][2] if v in new else ll[v] for v in range(n)]
        params_new = params + sum((k[v] - 1) * (new[v][1] - rows[v]) for v in new)
        now = pb.score(ll_new, params_new)
        before = len(uphill)
        accept = _accept(sched, rng, now, current, temperature, uphill)
        trace.append((method, frm, to, bits(now), accept))
        if len(uphill) == before:
            note("downhill_accept")
        else:
            note("uphill_accept" if accept else "uphill_reject")
        if accept:
            note(("add_accepted", "delete_accepted", "reverse_accepted")[method])
            for v, (mask, r, x) in new.items():
                pm[v], rows[v], ll[v] = mask, r, x
            params, current, no_changed = params_new, now, 0
            accepted += 1
            if len(lst) > 64:      # the copies go 64 entries per trip
                note("copy_gt64_accept")
            kept = list(lst)
        else:
            if len(kept) > 64:
                note("copy_gt64_reject")
            lst = list(kept)
            no_changed += 1
        note(("add_operated", "delete_operated", "reverse_operated")[method])
        temperature *= sched.rate
    flags = _flags(sched, temperature, no_changed, proposals)
    for bit, name in ((END_TEMPERATURE, "end_temperature"), (END_SAME_STATE, "end_same_state"), (END_CAP, "end_cap")):
        if flags & bit:
            note(name)
    return {"eval": current, "proposals": proposals, "operated": operated, "accepted": accepted, "flags": flags, "masks": pm,
            "edges": lst, "trace": trace, "uphill": uphill, "ll": ll, "params": params, "longest_list": longest}


def exp_margin_ok(uphill):
    """The only arithmetic that may differ between the host and the device is exp: every uphill decision must have
    |u - p| > 2^-40 * p, or p < 2^-33 where both sides reject (u >= 2^-33)."""
    return all(p < 2.0 ** -33 or abs(u - p) > 2.0 ** -40 * p for u, p in uphill)


# ---- the fixed inputs of the CPU and the GPU tests --------------------------------------------------

_INPUTS = {}
INPUT_SPECS = {   # name: (nodes, generator's max_parents, window, arities, model seed, draws, sample seed)
    "n1": (1, 0, 1, [3], 1, 300, 11),
    "n2": (2, 1, 64, [2, 3], 2, 2049, 12),
    "n5": (5, 2, 64, [2, 3, 2, 4, 2], 3, 2049, 13),
    "n6": (6, 3, 64, [2, 1, 3, 4, 2, 5], 4, 2049, 14),
    "n33": (33, 3, 16, [2, 3, 2], 5, 2049, 15),
    "n64": (64, 2, 8, [2], 6, 2049, 16),
    "bigk": (4, 1, 64, [255, 255, 255, 2], 7, 500, 17),   # 255^3 > 2^20: families that are not eligible
}


def anneal_input(name):
    """(model, learning_refs.Table) of one fixed input; cached per process."""
    if name not in _INPUTS:
        from bayesiannetwork_amd import synth
        n, mp, window, k, mseed, draws, sseed = INPUT_SPECS[name]
        model = synth.random_dag(n, mp, window, k, seed=mseed)
        _INPUTS[name] = (model, LR.sample_table(model, draws, sseed))
    return _INPUTS[name]


def libm_term(table):
    """term(child, parents) over a learning_refs.Table with libm's logarithm; NaN for a family over 2^20 entries."""
    def term(child, parents):
        if int(table.k[child]) * math.prod(int(table.k[u]) for u in parents) > MAX_ENTRIES:
            return math.nan
        return table.libm_ll(child, parents)
    return term


PATH64 = [[]] + [[v - 1] for v in range(1, 64)]   # 0 -> 1 -> ... -> 63


def dense_start(n, degree):
    """Node v has the up to `degree` nodes before it as parents: 186 edges at n = 64, 93 at n = 33 (degree 3)."""
    return [list(range(max(0, v - degree), v)) for v in range(n)]


DENSE64, DENSE33, DENSE33_2 = dense_start(64, 3), dense_start(33, 3), dense_start(33, 2)
NEVER = 1 << 30   # a same_state_max no chain reaches

# name: (input, q, criterion, rule, initial_temp, final_temp, rate, boltzmann, same_state_max, max_proposals, chains, seed, start)
# The reference rule compares u with exp(-now / T): an uphill move needs a temperature of the order of the score, hence 1e4 .. 1e6.
RUNS = {
    "n1_cap": ("n1", 1, "aic", "reference", 1.0, 0.5, 0.9, 1.0, 100, 50, 1, 1, None),
    "n2_ref_aic": ("n2", 1, "aic", "reference", 3e4, 3e2, 0.8, 1.0, 100, 1 << 20, 4, 2, None),
    "n2_tie": ("n2", 1, "mdl", "metropolis", 1.0, 1e-3, 0.5, 1.0, 100, 2, 8, 26, None),   # chains 2 and 3 end in the same, best graph
    "n5_ref_aic": ("n5", 2, "aic", "reference", 1e5, 1e3, 0.9, 1.0, 100, 1 << 20, 5, 3, None),
    "n5_ref_mdl": ("n5", 2, "mdl", "reference", 1e5, 1e3, 0.9, 2.0, 100, 1 << 20, 4, 4, None),
    "n5_met_aic": ("n5", 2, "aic", "metropolis", 50.0, 0.5, 0.9, 1.0, 100, 1 << 20, 5, 5, None),
    "n5_met_mdl": ("n5", 2, "mdl", "metropolis", 50.0, 0.5, 0.9, 1.0, 100, 1 << 20, 4, 6, None),
    "n5_same_state": ("n5", 2, "mdl", "metropolis", 1e-3, 1e-9, 0.99, 1.0, 3, 1 << 20, 4, 7, None),
    "n5_cap": ("n5", 2, "aic", "metropolis", 50.0, 0.5, 0.999, 1.0, 100, 40, 4, 8, None),
    "n33_met_aic": ("n33", 3, "aic", "metropolis", 20.0, 0.2, 0.8, 1.0, 100, 1 << 20, 257, 9, None),
    "n33_ref_mdl": ("n33", 3, "mdl", "reference", 1e6, 1e4, 0.9, 1.0, 100, 1 << 20, 5, 10, None),
    "n64_path_met": ("n64", 2, "aic", "metropolis", 20.0, 0.2, 0.9, 1.0, 100, 1 << 20, 4, 11, PATH64),
    "n64_path_ref": ("n64", 2, "mdl", "reference", 1e6, 1e4, 0.9, 1.0, 100, 1 << 20, 5, 12, PATH64),
    "bigk_met": ("bigk", 3, "aic", "metropolis", 1e7, 1e5, 0.9, 1.0, 100, 1 << 20, 4, 13, None),
    # Long lists: the ordered erase moves 64 entries per round and the accept / reject copies go 64 per trip, so a dense start
    # (93 and 186 edges) puts tails of more than 64 and of more than 128 entries behind an erased edge.
    "n64_dense_met": ("n64", 3, "aic", "metropolis", 20.0, 0.2, 0.999, 1.0, NEVER, 250, 4, 31, DENSE64),
    "n64_dense_ref": ("n64", 3, "mdl", "reference", 1e6, 1e4, 0.98, 1.0, NEVER, 1 << 20, 4, 32, DENSE64),
    "n33_dense_ref": ("n33", 3, "aic", "reference", 1e6, 1e4, 0.98, 1.0, NEVER, 1 << 20, 4, 33, DENSE33),
    # the learner's bound (2) below the table's q (3): the refusal at in-degree 2 over rank tables sized for 3
    "n33_bound2_over_q3": ("n33", 3, "mdl", "metropolis", 20.0, 0.2, 0.98, 1.0, NEVER, 1 << 20, 4, 34, DENSE33_2),
    # Long chains: rate 0.9995, thousands of uphill decisions per chain.  (Every seed below passes exp_margin_ok on the CPU replay
    # over libm's terms; the GPU test asserts it again over the device's.)
    "n5_long_met": ("n5", 2, "aic", "metropolis", 50.0, 0.5, 0.9995, 1.0, NEVER, 1 << 20, 2, 35, None),
    "n6_long_ref": ("n6", 3, "mdl", "reference", 1e5, 1e3, 0.9995, 1.0, NEVER, 1 << 20, 2, 36, None),
}

# the learner's in-degree bound of a run where it is below the table's q: the Problem's q is the bound
MAX_PARENTS = {"n33_bound2_over_q3": 2}


def run_setup(name, term=None):
    """(Problem, Schedule, chains, seed) of one row of RUNS; `term`: the family terms (default: libm over the input's table)."""
    inp, q, criterion, rule, t0, t1, rate, boltz, same, cap, chains, seed, start = RUNS[name]
    model, table = anneal_input(inp)
    pb = Problem(table.k, MAX_PARENTS.get(name, q), criterion, table.total, term or libm_term(table), start)
    return pb, Schedule(t0, t1, rate, boltz, same, rule, cap), chains, seed
