"""bn_info_cond_pair_entropies / bn_info_cond_pair_counts (the conditional form of the all-pairs matrix-core kernel) against
tests/tree_refs.py: exact counts, closeness to the exact entropies, the header's bit rules and the refusals.

One table of 60 columns: arities drawn from 1..32 plus 33, 40 and 255, so that the slots of every width (32, 16, 8, 4, 2) cross the 64
and 128 slot-column boundaries over several tile rows.  P in {1, 63, 64, 65, 3000}; every pattern counts 1, 128 (two digit planes: the
u64-flush instantiation at small P) or 2^40.  The class is column 0 (arity 3, the lowest), 1 (arity 1), 30 (arity 2, middle), 31
(arity 33, middle) or 59 (arity 255, the highest; its states 7 and 250..254 never occur)."""
from decimal import Context, Decimal

import numpy as np
import pytest

import pattern_refs as R
import tree_refs as TR

pytestmark = pytest.mark.gpu

N_COLS = 60
CLASSES = [0, 1, 30, 31, 59]
SUBSET = [0, 1, 2, 3, 4, 6, 30, 31, 40, 57, 58, 59]      # 12 columns: every slot width, arity 1, and the wide 33, 40, 255
PS = [1, 63, 64, 65, 3000]
KINDS = {"unit": 1, "c128": 128, "c2p40": 1 << 40}
CASES = [(P, kind) for P in PS for kind in KINDS]
CTX = Context(prec=60)      # the arithmetic of the exact references


def arities():
    k = np.random.default_rng(41).integers(1, 33, N_COLS).astype(np.int32)
    k[[0, 1, 2, 3, 4, 5, 6, 30, 31, 40, 57, 58, 59]] = [3, 1, 32, 17, 9, 5, 2, 2, 33, 16, 4, 40, 255]
    return k


def host_table(P, kind):
    k = arities()
    rng = np.random.default_rng(1000 + P)
    pats = np.zeros((P, N_COLS), np.uint8)
    for c in range(N_COLS):
        if c == 59:
            ok = np.array([s for s in range(250) if s != 7])
            col = ok[rng.integers(0, len(ok), P)]
        else:
            col = rng.integers(0, int(k[c]), P)
            if c % 3 == 2:   # some dependence on the neighbour, so that the conditional information is not all noise
                col = np.where(rng.random(P) < 0.5, pats[:, c - 1] % int(k[c]), col)
        pats[:, c] = col
    return pats, np.full(P, KINDS[kind], np.uint64), k


class Shared:
    """Device tables and the library's results per (P, kind, class), made once and read by every test of the module."""

    def __init__(self):
        self.tables, self.results = {}, {}

    def table(self, P, kind):
        from bayesiannetwork_amd.evaluation import InfoTable
        if (P, kind) not in self.tables:
            pats, counts, k = host_table(P, kind)
            self.tables[(P, kind)] = (InfoTable(pats, counts, k, device=0), pats, counts, k)
        return self.tables[(P, kind)]

    def result(self, P, kind, cls):
        if (P, kind, cls) not in self.results:
            self.results[(P, kind, cls)] = self.table(P, kind)[0].cond_pair_entropies(cls)
        return self.results[(P, kind, cls)]

    def close(self):
        for t, _, _, _ in self.tables.values():
            t.close()


@pytest.fixture(scope="module")
def shared(bnlib):
    s = Shared()
    yield s
    s.close()


def features(cls):
    return [v for v in range(N_COLS) if v != cls]


def cells_of(pats, counts, k, cols):
    """The exact non-zero cells (uint64) of the joint table of the distinct columns among `cols`."""
    key = np.zeros(len(counts), np.int64)
    for c in sorted(set(cols)):
        key = key * int(k[c]) + pats[:, c].astype(np.int64)
    return TR.cells_by_key(key, counts)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("P,kind", CASES)
def test_exact_counts(shared, P, kind):
    t, pats, counts, k = shared.table(P, kind)
    for cls in CLASSES:
        sub = [v for v in SUBSET if v != cls]
        pairs = [(x, y) for x in sub for y in sub]                      # every ordered pair, the diagonal too
        got = t.cond_pair_counts(cls, pairs)
        assert t.last_pairs_ms() > 0.0 and t.info("cond_pairs_ns") > 0
        for (x, y), blk in zip(pairs, got):
            assert np.array_equal(blk, TR.cond_counts(pats, counts, k, x, y, cls)), (cls, x, y)
        if cls == 59:
            assert not got[0][7].any() and not got[0][250:].any()       # the states of the class that never occur


@pytest.mark.parametrize("P,kind", CASES)
def test_close_to_the_exact_entropies(shared, P, kind):
    t, pats, counts, k = shared.table(P, kind)
    for cls in CLASSES:
        kz, feats = int(k[cls]), features(cls)
        out = shared.result(P, kind, cls)
        cz = cells_of(pats, counts, k, [cls])
        hz = TR.entropy_exact_grouped(cz)
        assert out["hz"] == t.entropy([cls])                            # bit for bit
        assert abs(out["hz"] - hz) <= R.entropy_bound(hz, len(cz))
        hz_d = TR.entropy_exact_grouped(cz, rounded=False)
        p64 = pats.astype(np.int64)
        base = [p64[:, cls] * int(k[x]) + p64[:, x] for x in feats]       # the key of (class, x), built once per column
        one = [TR.cells_by_key(b, counts) for b in base]
        hxz_d = [TR.entropy_exact_grouped(c, rounded=False) for c in one]
        hxz = [float(h) for h in hxz_d]
        worst = 0.0
        for i, x in enumerate(feats):                                   # every pair, in every case
            assert abs(out["hxz"][i] - hxz[i]) <= TR.cond_entropy_bound(hxz[i], len(one[i]), kz), (cls, x)
            for j in range(i + 1, len(feats)):
                y = feats[j]
                c = TR.cells_by_key(base[i] * int(k[y]) + p64[:, y], counts)
                h_d = TR.entropy_exact_grouped(c, rounded=False)
                h = float(h_d)
                err = abs(out["hxyz"][i, j] - h)
                bound = TR.cond_entropy_bound(h, len(c), kz)
                worst = max(worst, err / bound)
                assert err <= bound, (cls, x, y, err, bound)
                # the exact value in 60-digit decimal: the reference has no rounding of its own
                exact_cmi = CTX.subtract(CTX.subtract(CTX.add(hxz_d[i], hxz_d[j]), h_d), hz_d)
                cb = TR.cmi_bound(hxz[i], len(one[i]), hxz[j], len(one[j]), h, len(c), hz, len(cz), kz)
                assert abs(CTX.subtract(Decimal(float(out["cmi"][i, j])), exact_cmi)) <= Decimal(cb), (cls, x, y)
        print(f"P={P} {kind} class {cls}: worst |hxyz - exact| / bound = {worst:.3g}")
        # the pairs of the 12-column subset against pattern_refs' own cells, and against the single calls
        sub = [v for v in SUBSET if v != cls]
        for a, x in enumerate(sub):
            for y in sub[a:]:
                i, j = feats.index(x), feats.index(y)
                c = R.cell_counts(pats, counts, [x, y, cls])
                h = TR.entropy_exact_grouped(c)
                assert h == TR.entropy_exact_grouped(cells_of(pats, counts, k, [x, y, cls]))
                if P <= 65:
                    assert h == TR.entropy_exact3(pats, counts, x, y, cls)
                two_routes = TR.cond_entropy_bound(h, len(c), kz) + R.entropy_bound(h, len(c))
                assert abs(out["hxyz"][i, j] - t.entropy([x, y, cls])) <= two_routes, (cls, x, y)
            c = R.cell_counts(pats, counts, [x, cls])
            h = TR.entropy_exact_grouped(c)
            i = feats.index(x)
            assert abs(out["hxz"][i] - t.entropy([x, cls])) <= TR.cond_entropy_bound(h, len(c), kz) + R.entropy_bound(h, len(c)), (cls, x)


@pytest.mark.parametrize("P,kind", CASES)
def test_bit_rules(shared, P, kind):
    from bayesiannetwork_amd.evaluation import InfoTable
    t, pats, counts, k = shared.table(P, kind)
    perm = np.random.default_rng(3).permutation(P)
    with InfoTable(pats[perm], counts[perm], k, device=0) as tp:
        for cls in CLASSES:
            feats = features(cls)
            out = shared.result(P, kind, cls)
            hxyz, hxz, cmi, hz = out["hxyz"], out["hxz"], out["cmi"], out["hz"]
            assert same_bits(hxyz, hxyz.T)
            assert same_bits(np.diag(hxyz), hxz)
            assert same_bits(cmi, hxz[:, None] + hxz[None, :] - hxyz - hz)
            again = t.cond_pair_entropies(cls)                           # the run
            perm_out = tp.cond_pair_entropies(cls)                       # the pattern order
            for key in ("hxz", "hxyz", "cmi"):
                assert same_bits(again[key], out[key]) and same_bits(perm_out[key], out[key]), (cls, key)
            assert again["hz"] == hz and perm_out["hz"] == hz
            # a subset in another order with a duplicate: m, the position and the duplicate change nothing
            sub = [v for v in reversed(SUBSET) if v != cls] + [SUBSET[2], 17]
            idx = [feats.index(v) for v in sub]
            part = t.cond_pair_entropies(cls, sub)
            assert same_bits(part["hxyz"], hxyz[np.ix_(idx, idx)]) and same_bits(part["hxz"], hxz[idx])
            assert same_bits(part["cmi"], cmi[np.ix_(idx, idx)]) and part["hz"] == hz
            no_cmi = t.cond_pair_entropies(cls, sub, cmi=False)
            assert "cmi" not in no_cmi and same_bits(no_cmi["hxyz"], part["hxyz"])
            # a pair with the arity-40 column has the bits of the single call
            if cls != 58:
                i = feats.index(58)
                for y in (2, 30 if cls != 30 else 31, 57, 58):
                    assert hxyz[i, feats.index(y)] == t.entropy([58, y, cls]), (cls, y)
            if int(k[cls]) == 1:                                         # a class of arity 1: the unconditional call's bits
                pe = t.pair_entropies(feats)
                assert same_bits(hxyz, pe["hxy"]) and same_bits(hxz, pe["h"]) and same_bits(cmi, pe["mi"])


def test_conditional_matrix_function(shared):
    from bayesiannetwork_amd.evaluation import conditional_mutual_information_matrix
    t = shared.table(65, "unit")[0]
    out = conditional_mutual_information_matrix(t, 30, [2, 3, 58])
    feats = features(30)
    idx = [feats.index(v) for v in (2, 3, 58)]
    assert same_bits(out["cmi"], shared.result(65, "unit", 30)["cmi"][np.ix_(idx, idx)])


def test_refusals(shared):
    from bayesiannetwork_amd import _lib
    import ctypes
    t, pats, counts, k = shared.table(64, "unit")
    lib = _lib.lib()
    i32, f64 = ctypes.c_int32, ctypes.c_double
    v = (i32 * 3)(2, 3, 4)
    hz, hxz, hxyz, cmi = f64(), (f64 * 3)(), (f64 * 9)(), (f64 * 9)()
    launches = t.info("cond_pairs_ns")

    def refused(code):
        assert code == -1 and lib.bn_last_error().decode() != ""

    refused(lib.bn_info_cond_pair_entropies(t._h, -1, 3, v, ctypes.byref(hz), hxz, hxyz, cmi))
    refused(lib.bn_info_cond_pair_entropies(t._h, N_COLS, 3, v, ctypes.byref(hz), hxz, hxyz, cmi))
    refused(lib.bn_info_cond_pair_entropies(t._h, 3, 3, v, ctypes.byref(hz), hxz, hxyz, cmi))           # cond among vars
    refused(lib.bn_info_cond_pair_entropies(t._h, 0, 0, v, ctypes.byref(hz), hxz, hxyz, cmi))
    refused(lib.bn_info_cond_pair_entropies(t._h, 0, -2, v, ctypes.byref(hz), hxz, hxyz, cmi))
    refused(lib.bn_info_cond_pair_entropies(t._h, 0, 3, None, ctypes.byref(hz), hxz, hxyz, cmi))
    refused(lib.bn_info_cond_pair_entropies(t._h, 0, 3, v, None, hxz, hxyz, cmi))
    refused(lib.bn_info_cond_pair_entropies(t._h, 0, 3, v, ctypes.byref(hz), None, hxyz, cmi))
    refused(lib.bn_info_cond_pair_entropies(t._h, 0, 3, v, ctypes.byref(hz), hxz, None, cmi))
    pr = (i32 * 2)(2, 3)
    cnt = (ctypes.c_uint64 * (255 * 32 * 17))()
    refused(lib.bn_info_cond_pair_counts(t._h, 60, 1, pr, cnt))
    refused(lib.bn_info_cond_pair_counts(t._h, 2, 1, pr, cnt))
    refused(lib.bn_info_cond_pair_counts(t._h, 0, 0, pr, cnt))
    refused(lib.bn_info_cond_pair_counts(t._h, 0, 1, pr, None))
    with pytest.raises(_lib.BnError):
        t.cond_pair_entropies(3, [2, 3])
    assert t.info("cond_pairs_ns") == launches                           # nothing ran
    out = t.cond_pair_entropies(0, [2, 3, 4])                            # the table still works
    assert same_bits(out["hxyz"], shared.result(64, "unit", 0)["hxyz"][np.ix_([1, 2, 3], [1, 2, 3])])
    assert np.array_equal(t.cond_pair_counts(0, [(2, 3)])[0], TR.cond_counts(pats, counts, k, 2, 3, 0))
