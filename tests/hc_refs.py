"""Plain Python restatement of the hierarchical-clustering structure search of include/bn_mi355x.h (bn_learn_hc) and a literal
transcription of the reference's loop (bayesian/learning/stepwise_structure_hc.hpp:131-360 over greedy.hpp:67-101).

The reference's header does not compile (it includes transinformation.hpp), so there is no oracle binary: `literal_run` is the
yardstick, line for line, with two stated differences -- a cluster has an id where the reference has a shared_ptr address (node
i's cluster is id i, merge number s makes id n + s; "smaller address" reads "smaller id"), and every draw comes from the
library's stream (run j owns anneal_refs.Stream(seed, j)).  `restated_run` is what the kernel does: parent masks, one stable
compaction per merge in place of the erases, no cycle check, no closing sweep.  tests/test_hc_refs.py holds the two equal and
shows the three facts that allow the shortcuts.

Both take `S`, an [n][n] array of doubles read as S[l][r] with l from the first cluster of make_similarity and r from the second;
the diagonal is never read."""
import math

import numpy as np

import anneal_refs as AR
import learning_refs as LR

ONE_CLUSTER, NO_SIMILARITY = 1, 2
bits = AR.bits


def canonical_bits(b):
    """The bits of a double as two machines can be asked to agree on them: every NaN reads as the one quiet NaN.  IEEE 754 leaves a
    NaN's sign and payload to the implementation -- inf - inf is 0xFFF8... on x86 and 0x7FF8... on the GPU, and which of two NaN
    operands an add hands on differs too -- and no step of the search can tell one NaN from another (every compare is false, every
    sum is NaN).  Any other value keeps its bits, the sign of a zero included."""
    b = int(b)
    return 0x7FF8000000000000 if (b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000 else b


def _f(x):
    return np.float64(x)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(_f(a) / _f(b))


def _pow(a, b):
    with np.errstate(all="ignore"):
        return float(np.power(_f(a), _f(b)))


def make_similarity(S, X, Y):
    """stepwise_structure_hc.hpp:240-259: one divide and one add per pair, X outer, Y inner."""
    count = float(len(X) * len(Y))
    value = 0.0
    for l in X:
        for r in Y:
            value += _div(S[l][r], count)
    return value


def first_maximum(values):
    """std::max_element with `<` (:223): best = 0; a later entry replaces it only when value[best] < value[i]."""
    best = 0
    for i in range(1, len(values)):
        if values[best] < values[i]:
            best = i
    return best


def first_maximum_keyed(values):
    """The same index from keys the kernel can reduce in any order: a NaN never replaces and is never replaced, so a NaN at index
    0 wins (key +inf, lowest index) and a NaN elsewhere never does (key -inf, and index 0 has a key at least that and a lower
    index).  The first index of the largest key."""
    best, best_key = -1, None
    for i, v in enumerate(values):
        key = (math.inf if i == 0 else -math.inf) if v != v else v
        if best < 0 or key > best_key:
            best, best_key = i, key
    return best


def _shuffle(rng, x):
    for i in range(len(x) - 1, 0, -1):
        j = rng.below(i + 1)
        x[i], x[j] = x[j], x[i]


def _flags(clusters, sims):
    return (ONE_CLUSTER if len(clusters) == 1 else 0) | (NO_SIMILARITY if not sims else 0)


# ---- the literal transcription -------------------------------------------------------------------

class _Cluster:
    def __init__(self, ident, nodes):
        self.id, self.nodes = ident, nodes


class _Graph:
    """graph_t as learn_with_hint uses it: add_edge (graph.hpp:268) with the library's two extra refusals, erase_edge."""

    def __init__(self, pb, facts):
        self.pb, self.n, self.facts = pb, pb.n, facts
        self.adj = [[False] * pb.n for _ in range(pb.n)]

    def in_vertexes(self, v):
        return [u for u in range(self.n) if self.adj[u][v]]

    def is_able_trace(self, a, b):
        if a == b:
            return True
        return any(self.adj[a][c] and self.is_able_trace(c, b) for c in range(self.n))

    def add_edge(self, frm, to):
        if self.is_able_trace(to, frm):
            self.facts["refused_cycle"] += 1
            return False
        if self.adj[frm][to]:
            self.facts["refused_existing"] += 1
            return False
        parents = sorted(self.in_vertexes(to) + [frm])
        if len(parents) > self.pb.q:
            self.facts["refused_q"] += 1
            return False
        x = self.pb.term(to, tuple(parents))
        if x != x:
            self.facts["refused_nan"] += 1
            return False
        self.adj[frm][to] = True
        return True

    def evaluate(self):   # sampling_.make_cpt(graph); eval_(graph)
        fam = [tuple(self.in_vertexes(v)) for v in range(self.n)]
        return self.pb.score([self.pb.term(v, fam[v]) for v in range(self.n)],
                             sum(LR.family_params(self.pb.k, v, fam[v]) for v in range(self.n)))


def literal_run(pb, S, alpha, seed, j):
    """pb: anneal_refs.Problem (q: the in-degree bound).  Returns the run's record and `facts`, the counts the shortcuts rest on."""
    n = pb.n
    rng = AR.Stream(seed, j)
    facts = {"refused_cycle": 0, "refused_existing": 0, "refused_q": 0, "refused_nan": 0, "sweep_removed": 0, "sims_over": 0}
    graph = _Graph(pb, facts)                                   # :134 erase_all_edge
    clusters = [_Cluster(i, [i]) for i in range(n)]             # :148-161
    next_id = [n]

    def make_similarity_tuple(lhs, rhs):                        # :240-259
        value = make_similarity(S, lhs.nodes, rhs.nodes)
        return [lhs, rhs, value] if lhs.id < rhs.id else [rhs, lhs, value]

    def is_related(sim, cluster):                               # :191
        return sim[0] is cluster or sim[1] is cluster

    def is_connected(sim, lhs, rhs):                            # :197
        lo, hi = (lhs, rhs) if lhs.id < rhs.id else (rhs, lhs)
        return sim[0] is lo and sim[1] is hi

    similarities = []                                           # :164-188
    average = 0.0
    max_edge_num = n * (n - 1) // 2
    for i in range(n):
        for k in range(i + 1, n):
            sim = make_similarity_tuple(clusters[i], clusters[k])
            average += _div(sim[2], float(max_edge_num))
            similarities.append(sim)

    merges = tried = kept = pruned = pairs_kept = 0
    merge_trace, prune_trace, decisions, draws = [], [], [], []
    while len(clusters) != 1 and similarities:                  # :267
        if len(similarities) > len(clusters) * (len(clusters) - 1) // 2:
            facts["sims_over"] += 1
        at = first_maximum([s[2] for s in similarities])        # :220-237
        result = list(similarities[at])
        del similarities[at]
        coin = rng.below(2)
        draws.append("coin")
        if coin:
            result[0], result[1] = result[1], result[0]
        parent, child, old_value = result
        merge_trace.append((parent.id, child.id, bits(old_value), coin))

        parent_nodes, child_nodes = list(parent.nodes), list(child.nodes)   # greedy.hpp:67 (by value)
        _shuffle(rng, child_nodes)
        draws.append(("children", len(child_nodes)))
        eval_now = graph.evaluate()
        for c in child_nodes:
            _shuffle(rng, parent_nodes)
            draws.append(("parents", len(parent_nodes)))
            for p in parent_nodes:
                if graph.add_edge(p, c):
                    tried += 1
                    eval_next = graph.evaluate()
                    if eval_next < eval_now:
                        eval_now = eval_next
                        kept += 1
                    else:
                        graph.adj[p][c] = False

        new_cluster = _Cluster(next_id[0], parent.nodes + child.nodes)      # :204-217
        next_id[0] += 1
        clusters.remove(parent)
        clusters.remove(child)
        clusters.append(new_cluster)
        merges += 1

        for cluster in list(clusters):                          # :299-348
            if cluster is new_cluster:
                continue
            connection, i = [], 0
            while i < len(similarities):
                if is_connected(similarities[i], cluster, parent) or is_connected(similarities[i], cluster, child):
                    connection.append(similarities[i])
                    del similarities[i]
                else:
                    i += 1
            new_similarity = make_similarity_tuple(new_cluster, cluster)
            if len(connection) == 2:
                probability = _pow(alpha, _div(new_similarity[2], average))
            elif len(connection) == 1:
                probability = _pow(alpha, _div(old_value, connection[0][2]))
            elif len(connection) == 0:
                prune_trace.append((cluster.id, 0, bits(new_similarity[2]), 0))
                continue
            else:
                raise RuntimeError("too connection")
            u = rng.uniform()
            draws.append("uniform")
            decisions.append((u, probability))
            if u < probability:
                pruned += 1
                prune_trace.append((cluster.id, len(connection), bits(new_similarity[2]), 1))
                continue
            pairs_kept += 1
            prune_trace.append((cluster.id, len(connection), bits(new_similarity[2]), 0))
            similarities.append(new_similarity)
        i = 0                                                   # :351-359
        while i < len(similarities):
            if is_related(similarities[i], parent) or is_related(similarities[i], child):
                del similarities[i]
                facts["sweep_removed"] += 1
            else:
                i += 1

    masks = [sum(1 << u for u in graph.in_vertexes(v)) for v in range(n)]
    return {"score": graph.evaluate(), "merges": merges, "tried": tried, "kept": kept, "pruned": pruned, "pairs_kept": pairs_kept,
            "flags": _flags(clusters, similarities), "masks": masks, "merge_trace": merge_trace, "prune_trace": prune_trace,
            "decisions": decisions, "draws": draws, "facts": facts,
            "sims": [(s[0].id, s[1].id, bits(s[2])) for s in similarities], "clusters": [c.id for c in clusters]}


# ---- what the kernel does ------------------------------------------------------------------------

def restated_run(pb, S, alpha, seed, j, events=None):
    def note(name, by=1):
        if events is not None:
            events[name] = events.get(name, 0) + by

    n, k = pb.n, pb.k
    rng = AR.Stream(seed, j)
    pm, rows = [0] * n, [1] * n
    ll = [pb.term(v, ()) for v in range(n)]
    params = sum(k[v] - 1 for v in range(n))
    nodes = {i: [i] for i in range(n)}
    clusters = list(range(n))
    sa, sb, sv = [], [], []
    average = 0.0
    for i in range(n):
        for r in range(i + 1, n):
            value = 0.0 + _div(S[i][r], 1.0)
            average += _div(value, float(n * (n - 1) // 2))
            sa.append(i), sb.append(r), sv.append(value)
    current = pb.score(ll, params)
    merges = tried = kept = pruned = pairs_kept = 0
    merge_trace, prune_trace, decisions, exponents = [], [], [], []
    while len(clusters) != 1 and sa:
        best = first_maximum_keyed(sv)
        if events is not None:   # what the pick had to decide: lane i % 64 scans the entries i, i + 64, ..., then the lanes are reduced
            keys = [(math.inf if i == 0 else -math.inf) if v != v else v for i, v in enumerate(sv)]
            again = [i for i in range(best + 1, len(sv)) if keys[i] == keys[best]]
            if again and len(sv) > 64:
                note("pick_tie_gt64")
            if again and again[0] % 64 != best % 64:
                note("pick_tie_other_lane")
            if again and len(sv) > 64 and any(i % 64 == best % 64 for i in again):
                note("pick_tie_same_lane")
            if sv[0] != sv[0]:
                note("pick_nan_index0")
            if any(v != v for v in sv[1:]):
                note("pick_nan_elsewhere")
        a, b, old_value = sa[best], sb[best], sv[best]
        coin = rng.below(2)
        parent, child = (b, a) if coin else (a, b)
        merge_trace.append((parent, child, bits(old_value), coin))
        x, y = list(nodes[child]), list(nodes[parent])
        _shuffle(rng, x)
        for c in x:
            _shuffle(rng, y)
            for p in y:
                if bin(pm[c]).count("1") >= pb.q:
                    note("refused_q")
                    continue
                mask = pm[c] | (1 << p)
                term = pb.term(c, AR._parents_of(mask))
                if term != term:
                    note("refused_nan")
                    continue
                tried += 1
                rows_new = rows[c] * k[p]
                params_new = params + (k[c] - 1) * (rows_new - rows[c])
                nxt = pb.score([term if v == c else ll[v] for v in range(n)], params_new)
                if nxt < current:
                    pm[c], rows[c], ll[c], params, current = mask, rows_new, term, params_new, nxt
                    kept += 1
        new = n + merges
        nodes[new] = nodes[parent] + nodes[child]
        clusters.remove(parent)
        clusters.remove(child)
        clusters.append(new)
        merges += 1
        # one stable compaction: the merged pair and every entry that joins a live cluster with parent or child leave the list
        with_parent, with_child = {}, {}
        ka, kb, kv = [], [], []
        for i in range(len(sa)):
            if i == best:
                continue
            dead_a, dead_b = sa[i] in (parent, child), sb[i] in (parent, child)
            if dead_a or dead_b:
                other, dead = (sb[i], sa[i]) if dead_a else (sa[i], sb[i])
                (with_parent if dead == parent else with_child)[other] = (i, sv[i])
            else:
                ka.append(sa[i]), kb.append(sb[i]), kv.append(sv[i])
        sa, sb, sv = ka, kb, kv
        for c in clusters[:-1]:
            new_value = make_similarity(S, nodes[new], nodes[c])
            conn = sorted(t[c] for t in (with_parent, with_child) if c in t)   # list order
            if len(conn) == 0:
                note("visit_0")
                prune_trace.append((c, 0, bits(new_value), 0))
                continue
            note("visit_%d" % len(conn))
            exponent = _div(new_value, average) if len(conn) == 2 else _div(old_value, conn[0][1])
            p = _pow(alpha, exponent)
            u = rng.uniform()
            decisions.append((u, p))
            exponents.append(exponent)
            if p != p:
                note("p_nan")
            elif p >= 1.0:
                note("p_ge1")
            elif p == 0.0:
                note("p_zero")
            if u < p:
                pruned += 1
                note("pruned")
                prune_trace.append((c, len(conn), bits(new_value), 1))
                continue
            pairs_kept += 1
            note("kept_pair")
            prune_trace.append((c, len(conn), bits(new_value), 0))
            sa.append(c), sb.append(new), sv.append(new_value)
    return {"score": current, "merges": merges, "tried": tried, "kept": kept, "pruned": pruned, "pairs_kept": pairs_kept,
            "flags": _flags(clusters, sa), "masks": pm, "merge_trace": merge_trace, "prune_trace": prune_trace,
            "decisions": decisions, "exponents": exponents, "ll": ll, "params": params,
            "sims": [(x, y, bits(v)) for x, y, v in zip(sa, sb, sv)], "clusters": clusters}


def cluster_plan(S, n, alpha, seed, j, exponents=None):
    """The clustering alone, as the reference's loop does it when BetweenLearning draws from an engine of its own: the stream gives
    the coin and the pruning uniforms only, and no pick, merge or pruning depends on the edges learned.  Returns (the (parent
    nodes, child nodes) of every learn_with_hint call in order, the (u, p) of every pruning decision); `exponents`: a list that
    takes every decision's exponent (what pow_margin_ok asks for)."""
    rng = AR.Stream(seed, j)
    nodes = {i: [i] for i in range(n)}
    clusters = list(range(n))
    sims, average = [], 0.0
    for i in range(n):
        for r in range(i + 1, n):
            value = make_similarity(S, [i], [r])
            average += _div(value, float(n * (n - 1) // 2))
            sims.append((i, r, value))
    calls, decisions = [], []
    while len(clusters) != 1 and sims:
        a, b, old_value = sims.pop(first_maximum([s[2] for s in sims]))
        parent, child = (b, a) if rng.below(2) else (a, b)
        calls.append((list(nodes[parent]), list(nodes[child])))
        new = n + len(calls) - 1
        nodes[new] = nodes[parent] + nodes[child]
        clusters.remove(parent)
        clusters.remove(child)
        clusters.append(new)
        for c in clusters[:-1]:
            joins = [s for s in sims if c in s[:2] and (parent in s[:2] or child in s[:2])]
            sims = [s for s in sims if s not in joins]
            new_value = make_similarity(S, nodes[new], nodes[c])
            if not joins:
                continue
            exponent = _div(new_value, average) if len(joins) == 2 else _div(old_value, joins[0][2])
            p = _pow(alpha, exponent)
            u = rng.uniform()
            decisions.append((u, p))
            if exponents is not None:
                exponents.append(exponent)
            if not u < p:
                sims.append((c, new, new_value))
    return calls, decisions


def pow_decision_clear(u, p, alpha, exponent):
    """One pruning decision u < p with p = pow(alpha, exponent): can the device's pow decide it otherwise?
      p is NaN        clear: u < NaN is false on both sides, the pair is kept
      p >= 1          clear: the largest u is 1 - 2^-33, both sides prune (+inf included)
      p == 0 exactly  clear BY EXACTNESS where 0 is one of pow's special cases: alpha = 0 with a positive exponent, or an infinite
                      exponent -- both sides return the same 0
      otherwise       |u - p| > 2^-40 * max(u, p).  A 0 from underflow is judged here and not above: the device may return a
                      subnormal in its place, and the rule holds for either because the smallest u is 2^-33 (what was clear
                      under this rule before the cases above were named stays clear)."""
    if p != p or p >= 1.0:
        return True
    if p == 0.0 and ((alpha == 0.0 and exponent > 0.0) or math.isinf(exponent)):
        return True
    return not abs(u - p) <= 2.0 ** -40 * max(u, p)


def pow_margin_ok(decisions, alpha=None, exponents=None):
    """The only arithmetic that may differ between the host and the device is pow: EVERY pruning decision of a run (its (u, p)
    and the exponent p came from) must be clear in the sense of pow_decision_clear.  Without the exponents only the NaN case and
    the margin can be judged (an infinite p then reads as unclear)."""
    if exponents is None:
        return all(p != p or not abs(u - p) <= 2.0 ** -40 * max(u, p) for u, p in decisions)
    assert len(decisions) == len(exponents)
    return all(pow_decision_clear(u, p, alpha, x) for (u, p), x in zip(decisions, exponents))


# ---- the fixed inputs of the CPU and the GPU tests --------------------------------------------------

_TINY = {"t1": (1, [3], 31), "t2": (2, [2, 3], 32), "t3": (3, [2, 3, 2], 33), "t4": (4, [3, 2, 2, 3], 34)}
_INPUTS = {}


def hc_input(name):
    """(model, learning_refs.Table): anneal_refs' inputs and four tiny ones of 1 .. 4 nodes (a chain with strong dependencies)."""
    if name == "bigk_counts":
        # bigk's arities over 255 weighted patterns (i, i, i, i % 2): an edge between two 255-state nodes pays for its 64 770
        # parameters, and the next candidate's family has 255^3 entries -- the NaN refusal.  (On bigk's own 500 samples no such
        # edge is ever kept, and no family of one parent is over the limit: the refusal cannot fire there.)
        if name not in _INPUTS:
            i = np.arange(255)
            pats = np.stack([i, i, i, i % 2], axis=1).astype(np.uint8)
            _INPUTS[name] = (None, LR.Table(pats, np.full(255, 1_000_000, np.uint64), [255, 255, 255, 2]))
        return _INPUTS[name]
    if name not in _TINY:
        return AR.anneal_input(name)
    if name not in _INPUTS:
        from bayesiannetwork_amd import synth
        n, k, seed = _TINY[name]
        model = synth.random_dag(n, 1, 1, k, seed=seed)
        _INPUTS[name] = (model, LR.sample_table(model, 1500, seed + 100))
    return _INPUTS[name]


def host_mi(table):
    """h[x] + h[y] - hxy[x][y] in fp64 over a learning_refs.Table: the device's matrix up to rounding (the CPU check of the seeds)."""
    n, total = table.n, float(table.total)

    def H(cols):
        _, inv = np.unique(table.pats[:, cols], axis=0, return_inverse=True)
        cells = np.zeros(int(inv.max()) + 1)
        np.add.at(cells, inv.ravel(), table.counts.astype(np.float64))
        p = cells[cells > 0] / total
        return float(0.0 - (p * np.log2(p)).sum())

    h = [H([x]) for x in range(n)]
    mi = np.zeros((n, n))
    for x in range(n):
        for y in range(x + 1, n):
            mi[x][y] = mi[y][x] = h[x] + h[y] - H([x, y])
    return mi


INF_TIES_PAIRS = ((1, 3), (4, 9), (8, 20), (15, 17), (20, 31))   # the +inf entries of "inf_ties" (n >= 32)
INF_TIES_NAN = (0, 2)                                             # its NaN: index 1 of the initial list
_KIND_IDS = {"sparse_nonfinite": 1, "nan_first": 1, "inf_ties": 2, "inf_sparse": 3}


def list_index(n, x, y):
    """Where the pair x < y sits in the initial list (row-major over the upper triangle)."""
    return x * (2 * n - x - 1) // 2 + y - x - 1


def _finite_entry(h):
    """A dyadic value in (0, 1) from a hash word, negative one time in eight: exact in every divide by a power of two."""
    v = (1 + (h >> 8) % 4093) / 4096.0
    return -v if (h >> 24) % 8 == 0 else v


def _nonfinite_matrix(kind, n):
    """A pure function of (kind, n): Philox4x32-10 on (x, y, kind id, 0) under the key (n, 0) decides every pair x < y.
      sparse_nonfinite  5 % NaN, 5 % +inf, 5 % -inf, else finite; S[0][1] finite
      nan_first         the same matrix with S[0][1] = NaN: the NaN at index 0 of the initial list wins the first pick
      inf_ties          finite but for +inf at INF_TIES_PAIRS (list indices in different lanes, more than 64 apart) and one NaN at
                        index 1: the first +inf wins the first pick, its merge of 1 and 3 takes (0, 1) out of the list, and
                        the NaN, now at index 0, wins the second
      inf_sparse        5 % +inf, else finite; no NaN and no -inf, so the initial average is +inf and not NaN
    Any NaN among the initial similarities (or +inf next to -inf) makes their average NaN, and then a visit with two connections
    has p = pow(alpha, x / NaN) = NaN and keeps its pair -- unless alpha = 1, where pow gives 1 and every visit prunes.  Starting
    from the complete list every visit has two connections until something is pruned, so under the first three kinds a run
    keeps every pair (alpha != 1) or cuts every pair (alpha = 1).  inf_sparse is the matrix with non-finite entries whose runs
    do both: finite / +inf = 0 gives p = 1 (prune), +inf / +inf = NaN keeps, and the visits with one connection that follow see
    +inf / finite = +-inf: pow's exact 0 and +inf."""
    S = np.zeros((n, n))
    for x in range(n):
        for y in range(x + 1, n):
            h = AR.philox4x32_10((x, y, _KIND_IDS[kind], 0), (n, 0))
            v = _finite_entry(h[1])
            if kind in ("sparse_nonfinite", "nan_first"):
                r = h[0] % 100
                v = math.nan if r < 5 else math.inf if r < 10 else -math.inf if r < 15 else v
            elif kind == "inf_sparse" and h[0] % 100 < 5:
                v = math.inf
            S[x][y] = S[y][x] = v
    if kind == "sparse_nonfinite" and not math.isfinite(S[0][1]):
        S[0][1] = S[1][0] = 0.5
    elif kind == "nan_first":
        S[0][1] = S[1][0] = math.nan
    elif kind == "inf_ties":
        for x, y in INF_TIES_PAIRS:
            S[x][y] = S[y][x] = math.inf
        S[INF_TIES_NAN[0]][INF_TIES_NAN[1]] = S[INF_TIES_NAN[1]][INF_TIES_NAN[0]] = math.nan
    return S


def similarity_matrix(kind, n, mi=None):
    """"mi": the mutual information; the others are a caller's matrix (symmetric in bits)."""
    if kind == "mi":
        return mi
    if kind in _KIND_IDS:
        return _nonfinite_matrix(kind, n)
    S = np.zeros((n, n))
    if kind == "zero":
        return S
    for x in range(n):
        for y in range(x + 1, n):
            if kind == "ties":
                S[x][y] = S[y][x] = 0.25 if (x + y) % 2 else 0.5     # many equal maxima: the first in list order wins
            elif kind == "negative":
                S[x][y] = S[y][x] = 0.125 * (1 + (3 * x + 5 * y) % 7)
    if kind == "negative":
        S[0][n - 1] = S[n - 1][0] = -0.375
    return S


# name: (input, q, criterion, alpha, runs, seed, similarity kind).  Every seed was chosen so that the replay over libm terms and
# the host's mutual information passes pow_margin_ok (tests/test_hc_refs.py asserts it).
RUNS = {
    "t1": ("t1", 1, "aic", 0.5, 2, 1, "mi"),
    "t2": ("t2", 1, "mdl", 0.5, 4, 2, "mi"),
    "t2_tie": ("t2", 1, "aic", 0.0, 8, 3, "ties"),
    "t3": ("t3", 2, "aic", 0.5, 8, 4, "mi"),
    "t4_mid": ("t4", 2, "mdl", 0.5, 16, 5, "mi"),
    "n5_mid": ("n5", 2, "aic", 0.5, 16, 6, "mi"),
    "n5_alpha0": ("n5", 2, "mdl", 0.0, 4, 7, "mi"),
    "n5_alpha1": ("n5", 2, "aic", 1.0, 4, 8, "mi"),
    "t3_alpha1": ("t3", 2, "mdl", 1.0, 4, 17, "mi"),
    "n6_q1": ("n6", 1, "aic", 0.3, 8, 9, "mi"),
    "n6_q2": ("n6", 2, "mdl", 0.3, 8, 10, "mi"),
    "bigk": ("bigk", 3, "aic", 0.2, 4, 11, "mi"),
    "bigk_counts": ("bigk_counts", 3, "aic", 0.2, 4, 18, "mi"),
    # (node 32 of n33 has no parent and no child in the generating network -- its largest mutual information is 0.002 bits -- so no
    # seed or alpha makes it keep an edge: n33 shows ranked masks with bit 32 and the refusal at in-degree 3, n64 kept masks past bit 31)
    "n33": ("n33", 3, "mdl", 0.4, 6, 12, "mi"),
    "n64": ("n64", 2, "aic", 0.3, 8, 13, "mi"),
    "n5_ties": ("n5", 2, "aic", 0.5, 4, 14, "ties"),
    "n5_zero": ("n5", 2, "aic", 0.5, 4, 15, "zero"),
    "n5_negative": ("n5", 2, "mdl", 0.5, 8, 16, "negative"),
    # Lists of more than 64 entries (528 at n = 33, 2 016 at n = 64), where a lane scans several strided entries and equal maxima
    # sit in different lanes and in different slots of one lane; and a caller's non-finite matrices (_nonfinite_matrix), which
    # put NaN, +-inf and 0 exponents through pow at alpha 0, 0.5, 1 and 2
    "n33_ties": ("n33", 3, "aic", 0.5, 3, 40, "ties"),
    "n64_ties": ("n64", 2, "mdl", 0.5, 2, 41, "ties"),
    "n33_ties_alpha0": ("n33", 3, "mdl", 0.0, 2, 42, "ties"),
    "n33_ties_bound2": ("n33", 3, "aic", 0.5, 2, 43, "ties"),
    "n33_sparse": ("n33", 3, "aic", 0.5, 2, 44, "sparse_nonfinite"),
    "n33_nan_first": ("n33", 3, "mdl", 0.5, 2, 45, "nan_first"),
    "n33_inf_ties": ("n33", 3, "aic", 0.5, 2, 46, "inf_ties"),
    "n33_sparse_alpha0": ("n33", 3, "mdl", 0.0, 2, 47, "sparse_nonfinite"),
    "n33_sparse_alpha1": ("n33", 3, "aic", 1.0, 2, 48, "sparse_nonfinite"),
    "n33_sparse_alpha2": ("n33", 3, "mdl", 2.0, 2, 49, "sparse_nonfinite"),
    "n64_inf_ties": ("n64", 2, "aic", 0.5, 2, 50, "inf_ties"),
    "n33_inf_sparse": ("n33", 3, "aic", 0.5, 3, 51, "inf_sparse"),
    "n33_inf_sparse_alpha0": ("n33", 3, "mdl", 0.0, 2, 52, "inf_sparse"),
    "n33_inf_sparse_alpha2": ("n33", 3, "aic", 2.0, 2, 53, "inf_sparse"),
}
NEW_ROWS = tuple(list(RUNS)[list(RUNS).index("n33_ties"):])   # the rows of the long lists and the non-finite matrices


# the in-degree bound of a run where it is below the table's q.  On n6's samples no node ever earns a second parent (the largest
# mutual information but one is 0.026 bits), so a refusal AT in-degree 2 cannot be shown there: the q = 2 run bounds the in-degree
# at 1 over the q = 2 table, which is the kernel's other path -- the bound and the rank tables differ.
# n33 does earn second and third parents (the n33 row refuses at in-degree 3): its bounded row refuses at in-degree 2.
MAX_PARENTS = {"n6_q2": 1, "n33_ties_bound2": 2}


def run_setup(name, term=None, mi=None):
    """(Problem, S, alpha, runs, seed) of one row of RUNS; the Problem's q is the run's in-degree bound.  term: the family terms (default: libm over the input's table); mi: the
    mutual-information matrix (default: host_mi)."""
    inp, q, criterion, alpha, runs, seed, kind = RUNS[name]
    _, table = hc_input(inp)
    pb = AR.Problem(table.k, MAX_PARENTS.get(name, q), criterion, table.total, term or AR.libm_term(table))
    if kind == "mi" and mi is None:
        mi = host_mi(table)
    return pb, similarity_matrix(kind, table.n, mi), alpha, runs, seed
