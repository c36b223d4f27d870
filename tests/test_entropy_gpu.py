"""Entropy and all-pairs mutual information on the GPU (bn_info_*, bayesiannetwork_amd.evaluation) against
the numpy fp64 restatement of transinformation.hpp:14-84, exact joint counts against np.bincount, and the
bit rules: hxy symmetric, every entry the bits of its single entropy({x, y}) call, results independent of
run and of pattern order."""
import os
import subprocess

import numpy as np
import pytest

from test_entropy_host import ROOT, build_cpp, np_entropy

pytestmark = pytest.mark.gpu

ARITIES = [1, 2, 3, 4, 5, 8, 16, 17, 33, 255]
COUNTS = {"one": lambda r, P: np.ones(P, np.uint64),
          "127": lambda r, P: np.full(P, 127, np.uint64),
          "128": lambda r, P: np.full(P, 128, np.uint64),
          "2^31": lambda r, P: np.full(P, 1 << 31, np.uint64),
          "2^40": lambda r, P: np.full(P, 1 << 40, np.uint64),
          "mixed": lambda r, P: r.choice(np.array([1, 127, 128, (1 << 31) - 1, 1 << 31, 1 << 40], np.uint64), P)}


def table(P, counts="one", seed=0, arities=ARITIES):
    r = np.random.default_rng(seed)
    k = np.array(arities, np.int32)
    pats = np.stack([r.integers(0, kk, P) for kk in k], axis=1).astype(np.uint8)
    return pats, COUNTS[counts](r, P), k


def np_bincount(pats, counts, x, y, kx, ky):
    out = np.zeros(kx * ky, np.uint64)
    np.add.at(out, pats[:, x].astype(np.int64) * ky + pats[:, y], counts)
    return out.reshape(kx, ky)


def close(a, b):
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 3000])
@pytest.mark.parametrize("counts", sorted(COUNTS))
def test_entropies_match_restatement(bnlib, P, counts):
    from bayesiannetwork_amd.evaluation import InfoTable
    pats, c, k = table(P, counts, seed=P)
    n = len(k)
    with InfoTable(pats, c, k, device=0) as t:
        r = t.pair_entropies()
        for x in range(n):
            assert close(t.entropy(x), np_entropy(pats, c, [x]))
            assert close(r["h"][x], np_entropy(pats, c, [x]))
            for y in range(n):
                assert close(r["hxy"][x, y], np_entropy(pats, c, [x, y])), (x, y)
        assert t.entropy(0) == 0.0   # an arity-1 column
        assert t.info("digit_passes") == max(1, (int(c.max()).bit_length() + 6) // 7)


@pytest.mark.parametrize("counts", ["one", "mixed"])
def test_pair_counts_equal_bincount(bnlib, counts):
    from bayesiannetwork_amd.evaluation import InfoTable
    pats, c, k = table(777, counts, seed=3)
    n = len(k)
    pairs = [(x, y) for x in range(n) for y in range(n)]
    with InfoTable(pats, c, k, device=0) as t:
        blocks = t.pair_counts(pairs)
    for (x, y), b in zip(pairs, blocks):
        assert b.shape == (k[x], k[y])
        assert np.array_equal(b, np_bincount(pats, c, x, y, k[x], k[y])), (x, y)


def test_hxy_bits_symmetric_and_single_call(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    r = np.random.default_rng(5)
    k = np.array(list(r.integers(1, 33, 60)) + [33, 40, 255], np.int32)   # many slot widths, a few wide columns
    pats = np.stack([r.integers(0, kk, 4000) for kk in k], axis=1).astype(np.uint8)
    c = r.integers(1, 1000, 4000).astype(np.uint64)
    with InfoTable(pats, c, k, device=0) as t:
        out = t.pair_entropies()
        h, hxy, mi = out["h"], out["hxy"], out["mi"]
        assert np.array_equal(hxy.view(np.uint64), hxy.T.view(np.uint64))
        assert np.array_equal(np.diag(hxy).view(np.uint64), h.view(np.uint64))
        m = len(k)
        for x, y in list(zip(r.integers(0, m, 40), r.integers(0, m, 40))) + [(60, 61), (62, 5), (3, 3), (62, 62)]:
            single = t.entropy([int(x), int(y)])
            assert hxy[x, y] == single, (x, y, hxy[x, y], single)
            assert mi[x, y] == h[x] + h[y] - hxy[x, y]
            assert close(single, np_entropy(pats, c, [x, y]))
        # a subset in another order, with a duplicate: the same bits
        sel = [7, 62, 7, 0, 33]
        sub = t.pair_entropies(sel)
        for i, x in enumerate(sel):
            for j, y in enumerate(sel):
                assert sub["hxy"][i, j] == hxy[x, y]


def test_bits_repeat_and_ignore_pattern_order(bnlib):
    from bayesiannetwork_amd.evaluation import InfoTable
    pats, c, k = table(5000, "mixed", seed=11)
    perm = np.random.default_rng(1).permutation(len(c))
    with InfoTable(pats, c, k, device=0) as t:
        a, b = t.pair_entropies(), t.pair_entropies()
        e1 = [t.entropy(s) for s in ([1, 2, 3], [4, 5, 6, 7], [2, 3, 4, 5, 6, 7, 8])]
    with InfoTable(pats[perm], c[perm], k, device=0) as t:
        p = t.pair_entropies()
        e2 = [t.entropy(s) for s in ([1, 2, 3], [4, 5, 6, 7], [2, 3, 4, 5, 6, 7, 8])]
    for key in ("h", "hxy", "mi"):
        assert np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64))
        assert np.array_equal(a[key].view(np.uint64), p[key].view(np.uint64))
    assert e1 == e2


def test_sets_dense_and_key_routes(bnlib):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.evaluation import InfoTable
    pats, c, k = table(20000, "mixed", seed=2)
    r = np.random.default_rng(4)
    with InfoTable(pats, c, k, device=0) as t:
        for size in range(3, 9):
            for _ in range(3):
                s = sorted(r.choice(len(k), size, replace=False).tolist())
                want = np_entropy(pats, c, s)
                cells = int(np.prod(k[s].astype(object)))
                key = t.entropy(s, route=2)
                assert close(key, want), (s, key, want)
                if cells <= 1 << 22:
                    assert t.entropy(s, route=1) == key   # one summation order on both routes
        wide = [9, 8, 7, 6, 5]                               # 255 * 33 * 17 * 16 * 8 cells > 2^22: the key route by default
        assert close(t.entropy(wide), np_entropy(pats, c, wide))
        assert t.entropy([3, 2, 3, 2]) == t.entropy([2, 3])  # sorted, duplicates dropped
        with pytest.raises(_lib.BnError) as ei:
            t.entropy(wide, route=1)
        assert ei.value.code == _lib.BN_ERR_ARG
    # a key of more than 64 bits: 9 columns of arity 255 (72 bits)
    r2 = np.random.default_rng(8)
    k9 = np.full(9, 255, np.int32)
    p9 = r2.integers(0, 255, (50, 9)).astype(np.uint8)
    with InfoTable(p9, np.ones(50, np.uint64), k9, device=0) as t:
        assert close(t.entropy(list(range(8))), np_entropy(p9, np.ones(50, np.uint64), list(range(8))))  # 64 bits: fine
        with pytest.raises(_lib.BnError) as ei:
            t.entropy(list(range(9)))
        assert ei.value.code == _lib.BN_ERR_ARG and "64 bits" in str(ei.value)


def test_state_out_of_range_then_usable(bnlib):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.evaluation import InfoTable
    pats, c, k = table(1000, "one", seed=6)
    bad = pats.copy()
    bad[517, 4] = k[4]
    with pytest.raises(_lib.BnError) as ei:
        InfoTable(bad, c, k, device=0)
    assert ei.value.code == _lib.BN_ERR_ARG and "out of range" in str(ei.value)
    with InfoTable(pats, c, k, device=0) as t:
        assert close(t.entropy([3, 4]), np_entropy(pats, c, [3, 4]))


def test_across_the_i32_flush_boundary(bnlib):
    """More than 2^24 patterns (the i32 accumulators are flushed between segments), unit and 2^31 counts."""
    from bayesiannetwork_amd.evaluation import InfoTable
    P = (1 << 24) + 4099
    r = np.random.default_rng(9)
    k = np.array([2, 3, 4], np.int32)
    pats = np.stack([r.integers(0, kk, P) for kk in k], axis=1).astype(np.uint8)
    for c in (np.ones(P, np.uint64), np.where(r.random(P) < 0.5, 1 << 31, 3).astype(np.uint64)):
        with InfoTable(pats, c, k, device=0) as t:
            blocks = t.pair_counts([(0, 1), (2, 0), (1, 2), (2, 2)])
            for (x, y), b in zip([(0, 1), (2, 0), (1, 2), (2, 2)], blocks):
                assert np.array_equal(b, np_bincount(pats, c, x, y, k[x], k[y]))
            out = t.pair_entropies()
            for x in range(3):
                for y in range(3):
                    assert out["hxy"][x, y] == t.entropy([x, y])
                    assert close(out["hxy"][x, y], np_entropy(pats, c, [x, y]))


def test_make_samples_round_trip(bnlib):
    from bayesiannetwork_amd import evaluation, synth
    from bayesiannetwork_amd.engine import LikelihoodWeighting, Sampler
    g = synth.random_dag(12, 3, 6, [2, 3, 4], seed=21)
    lw = LikelihoodWeighting(g, device=0, seed=5)
    table, _ = lw.make_samples(None, unit_size=20000, epsilon=0.02)
    s = Sampler()
    s.load_sample(table)
    keys = np.array(list(table.keys()), np.int64)
    cnt = np.array(list(table.values()), np.uint64)
    for x in range(g.n):
        assert close(evaluation.entropy(s, x), np_entropy(keys, cnt, [x]))
    assert close(evaluation.entropy(s, [0, 5, 7]), np_entropy(keys, cnt, [0, 5, 7]))
    hx, hy = evaluation.entropy(s, 2), evaluation.entropy(s, 9)
    assert evaluation.mutual_information(s, 2, 9) == hx + hy - evaluation.entropy(s, [2, 9])
    assert evaluation.mutual_information(s, 2, 9, hx, hy) == evaluation.mutual_information(s, 2, 9)
    mm = evaluation.mutual_information_matrix(s, range(g.n), k=g.k)
    for x in range(g.n):
        for y in range(g.n):
            assert close(mm["hxy"][x, y], np_entropy(keys, cnt, [x, y]))
    assert mm["hxy"][2, 9] == evaluation.entropy(s, [2, 9])
    assert evaluation.entropy(Sampler(), [0, 1]) == 0.0


def test_cpp_drop_in_overloads(bnlib, tmp_path):
    exe = build_cpp(tmp_path)
    p = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "evaluation gpu ok" in p.stdout
