"""Plain host references (numpy only) for the conditional all-pairs entropies and the tree learners, written independently of the
kernels:

- exact conditional counts N[z][x][y] of a column pair by np.add.at;
- H(X, Y, Z) from exact integer cells: pattern_refs.entropy_exact (60-digit decimal) over pattern_refs.cell_counts, and a form that
  takes one logarithm per DISTINCT cell value for sweeps over every pair (tests/test_tree_refs.py pins it to the other);
- the tolerances: cond_entropy_bound for an entry of hxyz / hxz, cmi_bound for an entry of cmi;
- kruskal(w, root): the maximum spanning tree under the library's edge order by Kruskal's algorithm (the kernel runs Prim's);
- all_trees(n): every labelled tree on n nodes from its Pruefer sequence."""
import decimal
import functools
import itertools

import numpy as np

import pattern_refs as R


# ---- conditional counts and entropies ------------------------------------------------------------------

def cond_counts(pats, counts, k, x, y, z):
    """The exact [k_z][k_x][k_y] uint64 counts of the patterns by (state of z, state of x, state of y)."""
    pats = np.asarray(pats)
    out = np.zeros((int(k[z]), int(k[x]), int(k[y])), np.uint64)
    np.add.at(out, (pats[:, z].astype(np.int64), pats[:, x].astype(np.int64), pats[:, y].astype(np.int64)), np.asarray(counts, np.uint64))
    return out


def cells_by_key(key, counts):
    """The exact non-zero cell sums (uint64) of `counts` grouped by the int64 `key` of each pattern: one sort."""
    order = np.argsort(key)
    ks = key[order]
    first = np.concatenate(([0], np.flatnonzero(ks[1:] != ks[:-1]) + 1))
    cells = np.add.reduceat(np.asarray(counts, np.uint64)[order], first)      # uint64 sums: exact
    return cells[cells > 0]


def entropy_exact3(pats, counts, x, y, z) -> float:
    """H(X, Y, Z) to fp64 from the exact cells (duplicates among x, y, z collapse)."""
    return R.entropy_exact(R.cell_counts(pats, counts, [x, y, z]))


_CTX = decimal.Context(prec=60)


_LN2 = _CTX.ln(decimal.Decimal(2))


@functools.lru_cache(maxsize=1 << 16)
def _ln(v: int):
    return _CTX.ln(decimal.Decimal(v))


def entropy_exact_grouped(cells, rounded: bool = True):
    """pattern_refs.entropy_exact with the cells grouped by value: (sum over distinct c of mult(c) c (ln N - ln c)) / (N ln 2) in
    60-digit decimal arithmetic, rounded once to fp64.  The same number (the decimal sums agree to ~58 digits), one ln per value, kept.
    rounded=False: the 60-digit Decimal itself, for differences of entropies that must carry no rounding of their own."""
    cells = np.asarray(cells, np.uint64).ravel()
    cells = cells[cells > 0]
    if cells.size == 0:
        return 0.0 if rounded else decimal.Decimal(0)
    vals, mult = np.unique(cells, return_counts=True)
    D = decimal.Decimal
    N = sum(int(v) * int(c) for v, c in zip(vals, mult))
    lnN = _ln(N)
    s = D(0)
    for v, c in zip(vals, mult):
        if int(v) != N:
            s = _CTX.add(s, _CTX.multiply(D(int(v) * int(c)), _CTX.subtract(lnN, _ln(int(v)))))
    h = _CTX.divide(s, _CTX.multiply(D(N), _LN2))
    return float(h) if rounded else h


def cond_entropy_bound(H, nnz, kz) -> float:
    """How far hxyz[x][y] = 0.0 + part_0 + ... + part_{kz - 1} may lie from the exact H(X, Y, Z).  Derived as
    pattern_refs.entropy_bound: every non-zero cell costs one division, log, product and addition (relative 2^-53 each, the log a few
    ulp), every term and partial sum is at most H + 2 in size -- and the kz parts are added up by kz more additions."""
    return (nnz + kz + 8) * 2.0 ** -52 * (H + 2.0)


def cmi_bound(hxz_x, nnz_xz, hxz_y, nnz_yz, hxyz, nnz_xyz, hz, nnz_z, kz) -> float:
    """How far cmi = hxz[x] + hxz[y] - hxyz - hz (left to right) may lie from the exact value: the four entropies' own bounds (hz is the
    single call's, pattern_refs.entropy_bound) plus the three roundings of the additions, each relative 2^-53 of a partial result that
    is at most hxz_x + hxz_y + hxyz + hz in size."""
    own = (cond_entropy_bound(hxz_x, nnz_xz, kz) + cond_entropy_bound(hxz_y, nnz_yz, kz) + cond_entropy_bound(hxyz, nnz_xyz, kz)
           + R.entropy_bound(hz, nnz_z))
    return own + 3 * 2.0 ** -53 * (abs(hxz_x) + abs(hxz_y) + abs(hxyz) + abs(hz))


# ---- spanning trees --------------------------------------------------------------------------------------

def edge_key(w, u, v):
    """Sort key of the edge {u, v}: weight descending, then (min, max) ascending; -0.0 and 0.0 give equal keys."""
    return (-float(w) + 0.0, min(u, v), max(u, v))


def kruskal_edges(w):
    """The edges (lo, hi) of the maximum spanning tree of the complete graph under edge_key, in the order Kruskal accepts them.  Only
    the upper triangle of w is read."""
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    lo, hi = np.triu_indices(n, 1)
    order = np.lexsort((hi, lo, -w[lo, hi]))          # edge_key, vectorised (a float sort takes -0.0 and 0.0 as equal)
    edges = zip(lo[order].tolist(), hi[order].tolist())
    comp = list(range(n))

    def find(a):
        while comp[a] != a:
            comp[a] = comp[comp[a]]
            a = comp[a]
        return a
    out = []
    for lo, hi in edges:
        a, b = find(lo), find(hi)
        if a != b:
            comp[a] = b
            out.append((lo, hi))
            if len(out) == n - 1:
                break
    return out


def orient(n, edges, root):
    """parent [n] (int32, -1 at root) of the tree `edges` walked from `root`; a node the walk does not reach keeps -2."""
    adj = [[] for _ in range(n)]
    for a, b in edges:
        adj[a].append(b)
        adj[b].append(a)
    parent = np.full(n, -2, np.int32)
    parent[root] = -1
    todo = [root]
    while todo:
        u = todo.pop()
        for v in adj[u]:
            if parent[v] == -2:
                parent[v] = u
                todo.append(v)
    return parent


def kruskal(w, root):
    """parent [n] of the maximum spanning tree under the library's edge order, oriented from `root`."""
    n = np.asarray(w).shape[0]
    return orient(n, kruskal_edges(w), root)


def all_trees(n):
    """Every labelled tree on n nodes (n^(n - 2) of them) as a sorted tuple of edges (lo, hi), from its Pruefer sequence."""
    if n == 1:
        yield ()
        return
    if n == 2:
        yield ((0, 1),)
        return
    for seq in itertools.product(range(n), repeat=n - 2):
        degree = [1] * n
        for s in seq:
            degree[s] += 1
        edges = []
        for s in seq:
            leaf = min(v for v in range(n) if degree[v] == 1)
            edges.append((min(leaf, s), max(leaf, s)))
            degree[leaf] -= 1
            degree[s] -= 1
        a, b = [v for v in range(n) if degree[v] == 1]
        edges.append((a, b))
        yield tuple(sorted(edges))
