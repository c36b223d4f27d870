"""Plain numpy / Python restatement of the scoring contract of include/bn_mi355x.h (bn_score_*) and of the reference's
calc_likelihood / aic / mdl (bayesian/evaluation/basic_info_criteria.hpp:44-117, aic.hpp, mdl.hpp).

The device never takes a logarithm: L = math.log per CPT entry (libm, the bits of the host's std::log), and every
GPU result is L gathered and added in a stated order, which the functions here repeat addition by addition.
`exact_total` and the `reference_*` functions are order-free yardsticks (math.fsum / the reference's own loop)."""
import math

import numpy as np

SEG = 256      # row sums: segments of 256 consecutive node ids
LANES = 256    # node sums: partial sums, folded by halves


def log_table(model) -> np.ndarray:
    """L[q] = log(cpt[q]) with math.log (np.log differs from libm by an ulp on some inputs); log(0) = -inf."""
    return np.array([math.log(x) if x > 0.0 else -math.inf for x in model.cpt.tolist()], dtype=np.float64)


def entry_index(model, pats) -> np.ndarray:
    """[P][n] flat CPT entry each pattern shows at each node: cpt_off[v] + row * k[v] + state, first parent most significant."""
    pats = np.asarray(pats).reshape(-1, model.n).astype(np.int64)
    q = np.zeros(pats.shape, dtype=np.int64)
    for v in range(model.n):
        row = np.zeros(pats.shape[0], dtype=np.int64)
        for u in model.parents(v):
            row = row * int(model.k[u]) + pats[:, u]
        q[:, v] = int(model.cpt_off[v]) + row * int(model.k[v]) + pats[:, v]
    return q


def rows_ref(model, pats, nodes=None, L=None) -> np.ndarray:
    """ll[p] in the header's order: per segment (node id >> 8) the selected nodes in increasing id from +0.0, then the
    segment sums in increasing segment order from +0.0; segments without a selected node are skipped."""
    L = log_table(model) if L is None else L
    q = entry_index(model, pats)
    sel = sorted(range(model.n) if nodes is None else {int(v) for v in nodes})
    total = np.zeros(q.shape[0])
    for seg in sorted({v // SEG for v in sel}):
        acc = np.zeros(q.shape[0])
        for v in (v for v in sel if v // SEG == seg):
            acc = acc + L[q[:, v]]
        total = total + acc
    return total


def family_counts_ref(model, pats, counts) -> np.ndarray:
    """N[q]: samples (patterns weighted by their counts) showing entry q; exact uint64."""
    q = entry_index(model, pats)
    N = np.zeros(int(model.cpt_off[-1]), dtype=np.uint64)
    c = np.asarray(counts, dtype=np.uint64)
    for v in range(model.n):
        np.add.at(N, q[:, v], c)
    return N


def node_terms(model, N, L, v) -> np.ndarray:
    """double(N[q]) * L[q] of node v's entries in increasing q; an entry no sample shows contributes +0.0 (skipped)."""
    o0, o1 = int(model.cpt_off[v]), int(model.cpt_off[v + 1])
    n, l = N[o0:o1], L[o0:o1]
    t = np.zeros(o1 - o0)
    nz = n != 0
    with np.errstate(invalid="ignore"):
        t[nz] = n[nz].astype(np.float64) * l[nz]
    return t


def nodes_ref(model, N, L=None) -> np.ndarray:
    """ll_node[v] in the header's order: 256 partial sums (partial t takes the entries r = t, t + 256, ... in increasing
    r from +0.0; adding a skipped entry's +0.0 changes no bit, a partial sum is never -0.0), then folded by halves."""
    L = log_table(model) if L is None else L
    out = np.zeros(model.n)
    for v in range(model.n):
        t = node_terms(model, N, L, v)
        pad = np.zeros((len(t) + LANES - 1) // LANES * LANES)
        pad[:len(t)] = t
        part = np.zeros(LANES)
        for chunk in pad.reshape(-1, LANES):
            part = part + chunk
        s = LANES // 2
        while s > 0:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
        out[v] = part[0]
    return out


def exact_total(terms) -> float:
    """Correctly rounded sum (math.fsum); -inf if a term is -inf."""
    terms = [float(x) for x in terms]
    if any(x == -math.inf for x in terms):
        return -math.inf
    return math.fsum(terms)


def gamma(m: int) -> float:
    """gamma_m = m u / (1 - m u), u = 2^-53: the order-free bound on m roundings."""
    u = 2.0 ** -53
    return m * u / (1.0 - m * u)


def parameters_ref(model) -> int:
    return sum((int(model.k[v]) - 1) * math.prod(int(model.k[u]) for u in model.parents(v)) for v in range(model.n))


def reference_likelihood(model, table: dict, nodes=None) -> float:
    """basic_info_criteria.hpp:51-91, literally: per node a dict keyed by the (node, parents) part of each pattern summing
    the counts, then likelihood -= count * log(theta) over that dict (insertion order here; the reference's is unspecified).
    `table`: {pattern tuple: count}."""
    likelihood = 0.0
    for node in (range(model.n) if nodes is None else nodes):
        node = int(node)
        parent = [int(u) for u in model.parents(node)]
        statistics = {}
        for sample, count in table.items():
            cond = tuple((x, int(sample[x])) for x in sorted(set(parent + [node])))
            statistics[cond] = statistics.get(cond, 0) + int(count)
        for cond, count in statistics.items():
            cond = dict(cond)
            select = cond.pop(node)
            row = 0
            for u in parent:
                row = row * int(model.k[u]) + cond[u]
            theta = float(model.cpt[int(model.cpt_off[node]) + row * int(model.k[node]) + select])
            likelihood -= count * (math.log(theta) if theta > 0.0 else -math.inf)
    return likelihood


def reference_aic(model, table: dict, nodes=None) -> float:
    return reference_likelihood(model, table, nodes) + float(parameters_ref(model))   # (aic.hpp:21-26: parameters over the whole graph)


def reference_mdl(model, table: dict, nodes=None) -> float:
    likelihood = reference_likelihood(model, table, nodes)
    size = sum(int(c) for c in table.values())
    if size == 0:
        raise RuntimeError("Sampling is not finished yet.")   # (mdl.hpp:34)
    return likelihood + float(parameters_ref(model)) * (math.log2(size) / 2)


def likelihood_bound(model, N, L, nodes=None) -> float:
    """Order-free bound on |computed - exact| for -sum over `nodes` of sum_q N[q] L[q], however the terms are added:
    gamma_m * sum |terms|, m = non-zero terms + 1 (the double(N) conversion / product rounding)."""
    mags, m = [], 0
    for v in (range(model.n) if nodes is None else nodes):
        t = node_terms(model, N, L, int(v))
        t = t[t != 0]
        m += len(t)
        mags.extend(np.abs(t).tolist())
    return gamma(m + 1) * math.fsum(mags)


def table_dict(pats, counts) -> dict:
    d = {}
    for row, c in zip(np.asarray(pats).tolist(), np.asarray(counts).tolist()):
        d[tuple(row)] = d.get(tuple(row), 0) + int(c)
    return d
