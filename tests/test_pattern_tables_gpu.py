"""The pattern-table kernels against the plain host references of tests/pattern_refs.py, at the shapes where their
bookkeeping can go wrong: the all-pairs MFMA kernel over many 128 x 128 tiles (every ordered pair's exact counts,
entropies within a stated fp64 bound of a 60-digit value), 7-bit count digits up to bit 63, zero counts, the i32
flush at exactly 2^24 patterns, transposes over several column tiles up to n_vars = 2^23, the packed key at exactly
2^64 cells, and CPT fitting past the 4 096-entry LDS counters."""
import numpy as np
import pytest

from pattern_refs import (block, cell_counts, cpt_edge_model, entropy_bound, entropy_exact, fit_cpt_ref, onehot_offsets,
                          pair_count_matrix, pair_entropies_ref, random_patterns, tiled_pair_count_matrix, tiled_table)

pytestmark = pytest.mark.gpu

TILE = 128


def slot_layout(k):
    """{column: (first slot column, slot width)} and K, as bn_info.cpp's all_pairs lays out columns of arity <= 32:
    widths 32, 16, 8, 4, 2 in that order, the caller's order within a width."""
    width = [max(2, 1 << (int(a) - 1).bit_length()) for a in k]
    slots, K = {}, 0
    for w in (32, 16, 8, 4, 2):
        for u, a in enumerate(k):
            if a <= 32 and width[u] == w:
                slots[u] = (K, w)
                K += w
    return slots, K


def digit_passes(c):
    return max(1, (int(np.max(c)).bit_length() + 6) // 7)


def make_counts(kind, P, seed):
    r = np.random.default_rng(seed)
    if kind == "unit":
        return np.ones(P, np.uint64)
    if kind == "zeros":                                       # a third of the patterns count 0, the rest < 128
        c = r.integers(1, 128, P).astype(np.uint64)
        c[r.random(P) < 1 / 3] = 0
        return c
    # "bit63": mixed magnitudes, one count with bit 63 set, the total below 2^64
    c = r.choice(np.array([1, 2, 127, 128, 129, (1 << 31) - 1, 1 << 31, 1 << 40, (1 << 49) + 3], np.uint64), P)
    c[r.random(P) < 0.1] = 0
    c[P // 3] = np.uint64((1 << 63) + 987654321)
    assert int(c.astype(object).sum()) < 1 << 64
    return c


def benchmark_layout():
    """530 arity-4 columns: K = 2120 slot columns, Kpad = 2176 = 17 tile rows, the last tile 72/128 used."""
    return np.full(530, 4, np.int32)


def mixed_layout():
    """Each slot width's run of slots crosses a 128-column tile boundary and a 64-column wave boundary (32: [0, 160),
    16: [160, 320), 8: [320, 480), 4: [480, 640), 2: [640, 800); Kpad = 896, 7 tile rows), with arity-1 columns and
    the wide (> 32, dense per-pair route) arities 33, 128 and 255; the caller's order interleaves the widths."""
    r = np.random.default_rng(17)
    k = ([17, 32, 20, 25, 31] + [16, 9, 12, 16, 10, 11, 13, 14, 15, 9] + list(r.integers(5, 9, 20)) + list(r.integers(3, 5, 40))
         + [1, 2, 1, 2, 2, 1] + list(r.integers(1, 3, 74)) + [33, 128, 255])
    return np.array(k, np.int32)[r.permutation(len(k))]


LAYOUTS = {"benchmark": benchmark_layout, "mixed": mixed_layout}


def flat_blocks(M, k, pairs):
    off = onehot_offsets(k)
    return np.concatenate([M[off[x]:off[x + 1], off[y]:off[y + 1]].ravel() for x, y in pairs])


def assert_counts(t, M, k, pairs):
    blocks = t.pair_counts(pairs)
    if not np.array_equal(np.concatenate([b.ravel() for b in blocks]), flat_blocks(M, k, pairs)):
        for (x, y), b in zip(pairs, blocks):   # name the first pair that differs
            assert np.array_equal(b, block(M, k, x, y)), (x, y)


def assert_entropies(out, M, k, N):
    """hxy within the fp64 bound of the reference for every pair; h its diagonal; mi = h[x] + h[y] - hxy bit for bit."""
    h, hxy, mi = out["h"], out["hxy"], out["mi"]
    ref, nnz = pair_entropies_ref(M, k, N)
    bound = entropy_bound(ref, nnz)
    bad = np.argwhere(np.abs(hxy - ref) > bound)
    assert bad.size == 0, [(int(x), int(y), hxy[x, y], ref[x, y]) for x, y in bad[:5]]
    assert np.array_equal(hxy.view(np.uint64), hxy.T.view(np.uint64))
    assert np.array_equal(np.diag(hxy).view(np.uint64), h.view(np.uint64))
    assert np.array_equal((h[:, None] + h[None, :] - hxy).view(np.uint64), mi.view(np.uint64))


@pytest.mark.parametrize("counts", ["unit", "bit63", "zeros"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_all_pairs_across_tiles(bnlib, layout, counts):
    from bayesiannetwork_amd.evaluation import InfoTable
    k = LAYOUTS[layout]()
    _, K = slot_layout(k)
    assert -(-K // TILE) >= (17 if layout == "benchmark" else 7) and K % TILE != 0
    P = 3000 if layout == "benchmark" else 2500                 # not multiples of 64
    pats = random_patterns(k, P, seed=len(k))
    c = make_counts(counts, P, seed=P)
    N = int(c.astype(object).sum())
    M = pair_count_matrix(pats, c, k)
    n = len(k)
    with InfoTable(pats, c, k, device=0) as t:
        assert t.info("digit_passes") == {"unit": 1, "zeros": 1, "bit63": 10}[counts] == digit_passes(c)
        assert_counts(t, M, k, [(x, y) for x in range(n) for y in range(n)])
        out = t.pair_entropies()
    assert_entropies(out, M, k, N)
    # a few blocks against the 60-digit value directly
    r = np.random.default_rng(1)
    for x, y in [(0, 0), (0, n - 1), (n - 1, n - 1)] + [tuple(r.integers(0, n, 2)) for _ in range(30)]:
        exact = entropy_exact(block(M, k, x, y))
        assert abs(out["hxy"][x, y] - exact) <= entropy_bound(exact, int((block(M, k, x, y) > 0).sum())), (x, y)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bit_rules_across_tiles(bnlib, layout):
    """DESIGN 4.9's promises across tiles: hxy[x, y] has the bits of entropy([x, y]) for every pair touching a column
    whose slot starts or ends on a 32-column boundary (every 64 / 128 boundary among them), and a reordered subset
    with a duplicate, drawn from different tiles, has the bits of the full matrix."""
    from bayesiannetwork_amd.evaluation import InfoTable
    k = LAYOUTS[layout]()
    n = len(k)
    slots, _ = slot_layout(k)
    P = 2011
    pats = random_patterns(k, P, seed=5)
    c = make_counts("bit63", P, seed=6)
    mod = 32 if layout == "mixed" else TILE
    edge = sorted(u for u, (s, w) in slots.items() if s % mod == 0 or (s + w) % mod == 0)
    assert len(edge) >= 8
    with InfoTable(pats, c, k, device=0) as t:
        out = t.pair_entropies()
        hxy = out["hxy"]
        if layout == "mixed":
            pairs = {(min(x, y), max(x, y)) for x in edge for y in range(n)}
        else:   # the 128-boundary columns among themselves and with a spread of others
            others = list(range(0, n, 7))
            pairs = {(min(x, y), max(x, y)) for x in edge for y in edge + others}
        for x, y in sorted(pairs):
            assert hxy[x, y] == t.entropy([x, y]), (x, y)
        by_tile = sorted(slots, key=lambda u: slots[u][0])
        sel = [by_tile[-1], by_tile[0], by_tile[len(by_tile) // 2], by_tile[0], by_tile[len(by_tile) // 3]]
        sel += [u for u in range(n) if u not in slots][:2]          # wide columns, if any
        sub = t.pair_entropies(sel)
    assert len({slots[u][0] // TILE for u in sel if u in slots}) >= 3
    for i, x in enumerate(sel):
        assert sub["h"][i] == out["h"][x]
        for j, y in enumerate(sel):
            assert sub["hxy"][i, j] == hxy[x, y], (x, y)
            assert sub["mi"][i, j] == out["mi"][x, y], (x, y)


@pytest.mark.parametrize("rem", [0, 64])
def test_i32_bound_at_2_24_patterns(bnlib, rem):
    """P = 2^24, every count 127, column 0 constant: its cell holds 127 * 2^24 = 2 130 706 432, the largest sum the
    kernel variant without u64 flushes may see; rem = 64 adds one row of 64 patterns and takes the flushing variant."""
    from bayesiannetwork_amd.evaluation import InfoTable
    k = np.array([2, 4, 3, 32], np.int32)
    base = random_patterns(k, 4096, seed=3)
    base[:, 0] = 0
    bc = np.full(4096, 127, np.uint64)
    r = 1 << 12
    pats, c = tiled_table(base, bc, r, rem)
    assert len(c) == (1 << 24) + rem
    M = tiled_pair_count_matrix(base, bc, k, r, rem)
    N = 127 * len(c)
    assert int(M[0, 0]) == N
    n = len(k)
    with InfoTable(pats, c, k, device=0) as t:
        del pats, c
        assert t.info("digit_passes") == 1
        assert t.pair_counts([(0, 0)])[0][0, 0] == 127 * ((1 << 24) + rem)
        assert_counts(t, M, k, [(x, y) for x in range(n) for y in range(n)])
        out = t.pair_entropies()
        single = {(x, y): t.entropy([x, y]) for x in range(n) for y in range(x, n)}
    assert_entropies(out, M, k, N)
    assert out["h"][0] == 0.0
    for (x, y), e in single.items():
        assert out["hxy"][x, y] == e


def test_flush_with_several_tiles_and_two_digits(bnlib):
    """More than 2^24 patterns, counts up to 300 (two digit passes) and K = 194 slot columns (2 tile rows, 3 workgroups):
    the flush between segments and the off-diagonal tile together."""
    from bayesiannetwork_amd.evaluation import InfoTable
    k = np.array([32, 17, 32, 2, 25, 32, 32], np.int32)
    _, K = slot_layout(k)
    assert K == 194
    base = random_patterns(k, 4096, seed=8)
    bc = np.random.default_rng(9).integers(0, 301, 4096).astype(np.uint64)
    bc[7] = 300
    r, rem = 4097, 77
    pats, c = tiled_table(base, bc, r, rem)
    assert len(c) > 1 << 24
    M = tiled_pair_count_matrix(base, bc, k, r, rem)
    N = int(bc.astype(object).sum()) * r + int(bc[:rem].astype(object).sum())
    n = len(k)
    with InfoTable(pats, c, k, device=0) as t:
        del pats, c
        assert t.info("digit_passes") == 2
        assert_counts(t, M, k, [(x, y) for x in range(n) for y in range(n)])
        out = t.pair_entropies()
    assert_entropies(out, M, k, N)
    for x in range(n):
        for y in range(n):
            exact = entropy_exact(block(M, k, x, y))
            assert abs(out["hxy"][x, y] - exact) <= entropy_bound(exact, int((block(M, k, x, y) > 0).sum())), (x, y)


@pytest.mark.parametrize("n", [65, 129, 200])
def test_tables_wider_than_one_transpose_tile(bnlib, n):
    """The transpose's column tiles (64 columns each): pairs straddling columns 63/64 and 127/128, every column's entropy."""
    from bayesiannetwork_amd.evaluation import InfoTable
    r = np.random.default_rng(n)
    k = r.integers(1, 7, n).astype(np.int32)
    P = 1000
    pats = random_patterns(k, P, seed=n + 1)
    c = r.integers(1, 1 << 20, P).astype(np.uint64)
    N = int(c.astype(object).sum())
    M = pair_count_matrix(pats, c, k)
    near = sorted({v for v in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, n - 2, n - 1) if v < n})
    with InfoTable(pats, c, k, device=0) as t:
        assert_counts(t, M, k, [(x, y) for x in near for y in near])
        hs = [t.entropy(x) for x in range(n)]
        out = t.pair_entropies()
    for x in range(n):
        cells = cell_counts(pats, c, [x])
        exact = entropy_exact(cells)
        assert abs(hs[x] - exact) <= entropy_bound(exact, len(cells)), x
    assert_entropies(out, M, k, N)


def test_table_at_the_n_vars_limit(bnlib):
    """n_vars = 2^23 (the API's limit; 131 072 column tiles of the transpose), P = 2: each column's entropy is 0 or
    H(1/4, 3/4) as its two states agree or not."""
    from bayesiannetwork_amd.evaluation import InfoTable
    n = 1 << 23
    r = np.random.default_rng(23)
    k = r.integers(2, 256, n).astype(np.int32)
    pats = np.empty((2, n), np.uint8)
    pats[0] = r.integers(0, 1 << 30, n) % k
    differ = r.random(n) < 0.5
    pats[1] = np.where(differ, (pats[0].astype(np.int64) + 1) % k, pats[0])
    c = np.array([1, 3], np.uint64)
    h13 = entropy_exact([1, 3])
    cols = sorted({0, 1, 63, 64, 65, 127, 128, 65535 * 64, 65536 * 64 - 1, 65536 * 64, 65536 * 64 + 1, n - 65, n - 64, n - 2, n - 1}
                  | set(int(v) for v in r.integers(0, n, 200)))
    with InfoTable(pats, c, k, device=0) as t:
        assert t.info("n_vars") == n
        hs = {x: t.entropy(x) for x in cols}
        spread = cols[::4] + [n - 1]
        out = t.pair_entropies(spread)
        hxy_single = t.entropy([0, n - 1])
    for x in cols:
        want = h13 if differ[x] else 0.0
        assert abs(hs[x] - want) <= entropy_bound(want, 2), (x, hs[x], want)
    for i, x in enumerate(spread):
        assert out["h"][i] == hs[x]
        for j, y in enumerate(spread):
            want = h13 if (differ[x] or differ[y]) else 0.0
            assert abs(out["hxy"][i, j] - want) <= entropy_bound(want, 2), (x, y)
    assert out["hxy"][0, len(spread) - 1] == hxy_single


def test_key_route_at_exactly_2_64_cells(bnlib):
    """64 binary columns, or 16 of arity 16, make a key of exactly 2^64 cells (make_set's cells == 0, key_bits == 64):
    the key route against the 60-digit value; one more column of arity >= 2 is an argument error."""
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.evaluation import InfoTable
    k = np.array([2] * 64 + [16] * 16 + [2, 1], np.int32)
    P = 3000
    pats = random_patterns(k, P, seed=64)
    pats[:1000] = pats[0]                                    # one cell with many patterns
    c = make_counts("bit63", P, seed=65)
    bits, hex16 = list(range(64)), list(range(64, 80))
    mixed = list(range(4, 64)) + [64]                          # 2^60 * 16
    with InfoTable(pats, c, k, device=0) as t:
        got = {name: t.entropy(s) for name, s in (("bits", bits), ("hex16", hex16), ("mixed", mixed))}
        assert t.entropy(bits + [81]) == got["bits"]           # an arity-1 column adds no key digit
        assert t.entropy(bits, route=2) == got["bits"]
        for s, route in ((bits + [80], 0), (hex16 + [0], 0), (bits + [64], 2), (bits, 1), (hex16, 1)):
            with pytest.raises(_lib.BnError) as ei:                # more than 2^64 cells; 2^64 cells on the dense route
                t.entropy(s, route=route)
            assert ei.value.code == _lib.BN_ERR_ARG
    for name, s in (("bits", bits), ("hex16", hex16), ("mixed", mixed)):
        cells = cell_counts(pats, c, s)
        exact = entropy_exact(cells)
        assert abs(got[name] - exact) <= entropy_bound(exact, len(cells)), (name, got[name], exact)


@pytest.mark.parametrize("counts", ["zeros", "bit63"])
def test_dense_and_key_routes_on_zero_and_bit63_counts(bnlib, counts):
    from bayesiannetwork_amd.evaluation import InfoTable
    k = np.array([2, 3, 4, 5, 7, 16, 17, 33, 1, 255], np.int32)
    P = 5000
    pats = random_patterns(k, P, seed=10)
    c = make_counts(counts, P, seed=11)
    if counts == "zeros":
        c[pats[:, 9] == 254] = 0                               # state 254 of column 9 is seen only with count 0
    r = np.random.default_rng(12)
    sets = [[9], [8], [0, 8], [9, 7], [9, 6, 5], [0, 1, 2, 3, 4, 5]] + [sorted(r.choice(10, 3, replace=False).tolist()) for _ in range(8)]
    with InfoTable(pats, c, k, device=0) as t:
        got = [(t.entropy(s, route=1), t.entropy(s, route=2)) for s in sets]
    for s, (dense, key) in zip(sets, got):
        assert dense == key, s
        cells = cell_counts(pats, c, s)
        exact = entropy_exact(cells)
        assert abs(dense - exact) <= entropy_bound(exact, len(cells)), (s, dense, exact)


@pytest.mark.parametrize("P", [1, 1000, 5003])
def test_fit_cpt_at_the_lds_edge_and_beyond(bnlib, oracle_mod, P):
    """CPTs of exactly 4 096 entries (LDS counters) and 4 097 (global counters), 2^17 entries (16 binary parents),
    65 536 (three arity-16 parents), arity-255 nodes with a parent; counts up to ~2^62 with zeros; bit for bit
    against the numpy count and the C restatement."""
    from bayesiannetwork_amd.engine import fit_cpt
    m = cpt_edge_model()
    pats = random_patterns(m.k, P, seed=P + 1)
    pats[: min(P, 40)] = pats[0]                                # repeated patterns: many adds on one counter
    r = np.random.default_rng(P + 2)
    c = r.integers(0, 1 << 20, P).astype(np.uint64)
    c[r.random(P) < 0.1] = 0
    c[0] = np.uint64((1 << 62) + 5)
    if P > 2:
        c[P - 1] = np.uint64((1 << 62) - 3)
        c[P // 2] = np.uint64(1 << 61)
    fit = fit_cpt(m, pats, c, device=0)
    want = fit_cpt_ref(m, pats, c)
    bad = np.flatnonzero(fit.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, [(int(i), int(np.searchsorted(m.cpt_off, i, side="right") - 1), fit[i], want[i]) for i in bad[:5]]
    assert np.array_equal(fit, oracle_mod.make_cpt(m, pats, c))
    sizes = np.diff(m.cpt_off)
    assert 4096 in sizes and 4097 in sizes and sizes.max() == 1 << 17
