"""Plain host references for the pattern-table kernels (entropy / all-pairs counts of bn_info_*, CPT fitting of
bn_fit_cpt), written independently of the kernels and of numpy's fp64 log2:

- exact joint counts of every column pair at once: X^T diag(w) X over one-hot float64 operands, the counts split
  into 16-bit limbs so that every partial sum is an integer below 2^53 (exact in any summation order while
  P < 2^37), the limbs recombined in uint64;
- the counts of a table made by repeating a small base table, at the cost of the base;
- H = -sum (c/N) log2(c/N) from exact integer cells in `decimal` arithmetic at 60 digits, and a vectorised
  long-double form for the all-pairs sweep (pinned against the decimal one by tests/test_pattern_refs.py);
- the tolerance an fp64 sum of nnz terms may differ from the exact H by;
- sampler::make_cpt counted in uint64 with np.add.at."""
import decimal

import numpy as np

LIMB_BITS = 16


def onehot_offsets(k):
    """Row / column of state 0 of each column in the one-hot matrix (column c's states at off[c] .. off[c] + k[c])."""
    k = np.asarray(k, np.int64)
    return np.concatenate([[0], np.cumsum(k)])


def pair_count_matrix(pats, counts, k):
    """The exact [sum k][sum k] uint64 matrix of joint counts: entry (off[x] + i, off[y] + j) is the total count of
    the patterns with state i in column x and state j in column y."""
    pats = np.asarray(pats)
    counts = np.asarray(counts, np.uint64)
    P = len(counts)
    assert P < 1 << 37, "a limb product sum would pass 2^53"
    off = onehot_offsets(k)
    X = np.zeros((P, int(off[-1])), np.float64)
    rows = np.arange(P)
    for c in range(len(k)):
        X[rows, off[c] + pats[:, c].astype(np.int64)] = 1.0
    out = np.zeros((X.shape[1], X.shape[1]), np.uint64)
    for limb in range(64 // LIMB_BITS):
        part = (counts >> np.uint64(LIMB_BITS * limb)) & np.uint64((1 << LIMB_BITS) - 1)
        if not part.any():
            continue
        g = X.T @ (X * part.astype(np.float64)[:, None])          # integers < 2^53: exact
        out += np.rint(g).astype(np.uint64) << np.uint64(LIMB_BITS * limb)
    return out


def tiled_table(base_pats, base_counts, r, rem):
    """The table `base` repeated r times, then its first `rem` rows."""
    idx = np.concatenate([np.tile(np.arange(len(base_counts)), r), np.arange(rem)])
    return np.ascontiguousarray(base_pats[idx]), np.ascontiguousarray(base_counts[idx])


def tiled_pair_count_matrix(base_pats, base_counts, k, r, rem):
    """pair_count_matrix of tiled_table(base, r, rem), from the base alone."""
    full = pair_count_matrix(base_pats, base_counts, k) * np.uint64(r)
    return full + pair_count_matrix(base_pats[:rem], base_counts[:rem], k) if rem else full


def block(M, k, x, y):
    """The k[x] x k[y] joint counts of columns x and y out of a pair_count_matrix."""
    off = onehot_offsets(k)
    return M[off[x]:off[x + 1], off[y]:off[y + 1]]


def cell_counts(pats, counts, cols):
    """Exact non-zero cell counts (python ints) of the joint table of the columns `cols` (duplicates collapse)."""
    cols = sorted(set(int(c) for c in cols))
    counts = np.asarray(counts, np.uint64)
    if not cols:
        return [int(counts.sum(dtype=np.uint64))]
    _, inv = np.unique(np.asarray(pats)[:, cols], axis=0, return_inverse=True)
    cells = np.zeros(int(inv.max()) + 1, np.uint64)
    np.add.at(cells, inv.ravel(), counts)
    return [int(c) for c in cells if c]


_CTX = decimal.Context(prec=60)


def entropy_exact(cells) -> float:
    """H = -sum (c/N) log2(c/N) over the non-zero integer cells, as (sum c (ln N - ln c)) / (N ln 2) in 60-digit
    decimal arithmetic, rounded once to fp64."""
    cells = [int(c) for c in np.asarray(cells, dtype=object).ravel() if int(c) > 0]
    if not cells:
        return 0.0
    N = sum(cells)
    D = decimal.Decimal
    lnN = _CTX.ln(D(N))
    s = D(0)
    for c in cells:
        if c != N:
            s = _CTX.add(s, _CTX.multiply(D(c), _CTX.subtract(lnN, _CTX.ln(D(c)))))
    return float(_CTX.divide(s, _CTX.multiply(D(N), _CTX.ln(D(2)))))


def entropy_ld(blocks, N):
    """The same H for a stack of cell blocks [..., cells] (uint64) in long double, vectorised: -sum p log2 p with
    p = c / N (c and N exact in a 64-bit mantissa).  Where long double is fp64, this is an fp64 sum only."""
    c = np.asarray(blocks, np.uint64).astype(np.longdouble)
    p = c / np.longdouble(int(N))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(c > 0, -p * np.log2(np.where(c > 0, p, 1)), 0)
    return t.sum(axis=-1)


def entropy_bound(H, nnz) -> float:
    """How far an fp64 H = 0.0 - sum p log2 p over nnz non-zero cells may lie from the exact value: each of the nnz
    divisions, logs, products and additions rounds once (relative 2^-53 each, the log's error at most a few ulp),
    and every term and partial sum is at most H + 2 in size; (nnz + 8) * 2^-52 * (H + 2) covers that sum."""
    return (nnz + 8) * 2.0 ** -52 * (H + 2.0)


def pair_entropies_ref(M, k, N):
    """hxy [n][n] of every column pair from a pair_count_matrix (long double, then fp64) and nnz [n][n], the number of
    non-zero cells of each pair block."""
    k = np.asarray(k, np.int64)
    off = onehot_offsets(k)
    n = len(k)
    hxy = np.zeros((n, n), np.longdouble)
    nnz = np.zeros((n, n), np.int64)
    for a in np.unique(k):
        xs = np.flatnonzero(k == a)
        ri = (off[xs][:, None] + np.arange(a)).ravel()
        for b in np.unique(k):
            ys = np.flatnonzero(k == b)
            ci = (off[ys][:, None] + np.arange(b)).ravel()
            blk = M[np.ix_(ri, ci)].reshape(len(xs), a, len(ys), b).transpose(0, 2, 1, 3).reshape(len(xs), len(ys), a * b)
            hxy[np.ix_(xs, ys)] = entropy_ld(blk, N)
            nnz[np.ix_(xs, ys)] = (blk > 0).sum(axis=-1)
    return hxy.astype(np.float64), nnz


def fit_cpt_ref(model, pats, counts):
    """sampler::make_cpt: uint64 counts per (parent row, state), first parent the most significant row digit; each
    row count / float(row total), 1.0 / k for a row no pattern shows."""
    pats = np.asarray(pats, np.uint8).reshape(-1, model.n)
    counts = np.asarray(counts, np.uint64)
    out = np.zeros(int(model.cpt_off[-1]), np.float64)
    for v in range(model.n):
        kv = int(model.k[v])
        row = np.zeros(len(counts), np.int64)
        for u in model.in_idx[model.in_ptr[v]:model.in_ptr[v + 1]]:
            row = row * int(model.k[u]) + pats[:, u]
        size = int(model.cpt_off[v + 1] - model.cpt_off[v])
        cnt = np.zeros(size, np.uint64)
        np.add.at(cnt, row * kv + pats[:, v], counts)
        cnt = cnt.reshape(-1, kv)
        tot = cnt.sum(axis=1, dtype=np.uint64)
        seen = tot > 0
        rows = np.full(cnt.shape, 1.0 / kv)
        rows[seen] = cnt[seen].astype(np.float64) / tot[seen].astype(np.float64)[:, None]
        out[model.cpt_off[v]:model.cpt_off[v + 1]] = rows.ravel()
    return out


def cpt_edge_model():
    """A hand-built structure at the CPT fitting kernel's edges: CPTs of 2^17 entries (16 binary parents), 65 536 (three
    arity-16 parents), exactly 4 096 (the LDS counters' size) and 4 097 (one above: global counters), arity-255 nodes
    with a parent, and parents of unequal arities (the row's digit order matters)."""
    from bayesiannetwork_amd.flat import from_parent_lists
    k = [2] * 16 + [2] + [16] * 3 + [16] + [4] * 5 + [4] + [241, 17] + [255, 255, 255] + [3]
    parents = [[] for _ in range(len(k))]
    parents[16] = list(range(16))          # 2 * 2^16 = 131 072 entries
    parents[20] = [17, 18, 19]             # 16^4 = 65 536
    parents[26] = [21, 22, 23, 24, 25]     # 4 * 4^5 = 4 096
    parents[28] = [27]                     # 17 * 241 = 4 097
    parents[30] = [21]                     # 255 * 4 = 1 020
    parents[31] = [29]                     # 255 * 255 = 65 025
    parents[32] = [0, 17, 27]              # 3 * 2 * 16 * 241 = 23 136
    cpts = []
    for v, ps in enumerate(parents):
        rows = int(np.prod([k[u] for u in ps])) if ps else 1
        cpts.append(np.full(rows * k[v], 1.0 / k[v]))
    return from_parent_lists(k, parents, cpts, name="cpt_edges")


def random_patterns(k, P, seed):
    r = np.random.default_rng(seed)
    return np.stack([r.integers(0, kk, P) for kk in k], axis=1).astype(np.uint8)
