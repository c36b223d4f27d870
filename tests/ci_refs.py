"""Plain Python / libm restatement of the conditional-independence test of include/bn_mi355x.h (bn_ci_tests): exact counts
N[s][b][a], marginals, G in the stated order, both degrees-of-freedom rules and the chi-square tail chisq_sf as the header writes it.
numpy and math only."""
import math

import numpy as np

from bd_refs import lgamma_pos
from learning_refs import U, sum256
from loglik_refs import gamma

MAX_COND, MAX_CELLS = 8, 1 << 20
CHISQ_MAX_ITER, CHISQ_EPS, CHISQ_TINY = 100000, 2.0 ** -52, 2.0 ** -1000

# Worst relative error of chisq_sf below (libm log / exp) against the 50-digit values of tests/golden/chisq_sf.json, over the grid
# points whose tail is a normal double: measured 1.11e-10 (at df = 2^20, G = df + 2; 1.98e-11 at df = 65536; where the prefactor's exponent is a difference of terms of
# size ~7e6, each carrying a few 1e-16 relative; below 1e-12 elsewhere).  Asserted at four times that: the device's log / exp differ from libm's.
CHISQ_MEASURED = 1.11e-10
CHISQ_TOL = 4 * CHISQ_MEASURED
CHISQ_NORMAL = 1e-300     # below this the tail has (nearly) left the normal range: only 0 <= p <= CHISQ_NORMAL * (1 + tol) is asked


def counts(pats, weights, k, x, y, S) -> np.ndarray:
    """N[s][b][a], uint64 [strata][k_y][k_x]: s over the sorted S, first column most significant."""
    pats = np.asarray(pats).astype(np.int64)
    s = np.zeros(pats.shape[0], dtype=np.int64)
    strata = 1
    for u in sorted(int(v) for v in S):
        s = s * int(k[u]) + pats[:, u]
        strata *= int(k[u])
    kx, ky = int(k[x]), int(k[y])
    N = np.zeros(strata * ky * kx, dtype=np.uint64)
    np.add.at(N, (s * ky + pats[:, y]) * kx + pats[:, x], np.asarray(weights, dtype=np.uint64))
    return N.reshape(strata, ky, kx)


def marginals(N):
    """(N_s [strata], R [strata][k_y], C [strata][k_x]) as Python-int object arrays (exact beyond 2^53)."""
    N = np.asarray(N, dtype=np.uint64).astype(object)
    return N.sum(axis=(1, 2)), N.sum(axis=2), N.sum(axis=1)


def g_terms(N, log=math.log) -> np.ndarray:
    """t_r = double(N) * log((double(N) * double(N_s)) / (double(R) * double(C))) per cell r = (s * k_y + b) * k_x + a; 0.0 where N == 0."""
    N = np.asarray(N, dtype=np.uint64)
    Ns, R, C = marginals(N)
    t = np.zeros(N.shape)
    for s, b, a in zip(*np.nonzero(N)):
        n = float(int(N[s, b, a]))
        t[s, b, a] = n * log((n * float(Ns[s])) / (float(R[s, b]) * float(C[s, a])))
    return t.reshape(-1)


def g2(N, log=math.log) -> float:
    """G = 2.0 * (the terms in bn_score_nodes' order); not > 0.0 becomes +0.0."""
    g = 2.0 * sum256(g_terms(N, log))
    return g if g > 0.0 else 0.0


def g_bound(N) -> float:
    """|device G - 2 fsum(libm terms)| <= 2 (8u + gamma_{m+1}) sum |t|: the argument of the logarithm has the same bits on both sides
    (the same three IEEE operations on the same exact counts), the two logarithms are within 3 ulp of each other (6u relative), the
    product adds 2u, and m + 1 additions in any order add gamma_{m+1} -- learning_refs.ll_bound's derivation; the factor 2.0 is exact."""
    t = g_terms(N)
    m = int(np.count_nonzero(np.asarray(N)))
    return 2.0 * (8 * U + gamma(m + 1)) * math.fsum(np.abs(t).tolist())


def g_exact(N) -> float:
    return 2.0 * math.fsum(g_terms(N).tolist())


def df_nominal(N) -> int:
    strata, ky, kx = np.asarray(N).shape
    return (kx - 1) * (ky - 1) * strata


def df_adjusted(N) -> int:
    Ns, R, C = marginals(N)
    return sum((int(np.count_nonzero(R[s])) - 1) * (int(np.count_nonzero(C[s])) - 1) for s in range(len(Ns)) if Ns[s] != 0)


def df_of(N, rule) -> int:
    return df_adjusted(N) if rule in (1, "adjusted") else df_nominal(N)


def chisq_sf(g, df, log=math.log, exp=math.exp) -> float:
    """The header's chisq_sf, operation for operation."""
    g, df = float(g), int(df)
    if df <= 0 or not g > 0.0:
        return 1.0
    a, x = 0.5 * float(df), 0.5 * g
    e = ((a * log(x)) - x) - lgamma_pos(a, log)[0]
    pref = exp(e)
    if x < a + 1.0:
        ap, d = a, 1.0 / a
        total = d
        for _ in range(CHISQ_MAX_ITER):
            ap = ap + 1.0
            d = (d * x) / ap
            total = total + d
            if d < total * CHISQ_EPS:
                break
        q = 1.0 - (total * pref)
    else:
        b, c = (x + 1.0) - a, 1.0 / CHISQ_TINY
        d = 1.0 / b
        h = d
        for i in range(1, CHISQ_MAX_ITER + 1):
            an = (-float(i)) * (float(i) - a)
            b = b + 2.0
            d = (an * d) + b
            if abs(d) < CHISQ_TINY:
                d = CHISQ_TINY
            c = b + (an / c)
            if abs(c) < CHISQ_TINY:
                c = CHISQ_TINY
            d = 1.0 / d
            de = d * c
            h = h * de
            if abs(de - 1.0) < CHISQ_EPS:
                break
        q = pref * h
    if not q > 0.0:
        return 0.0
    return 1.0 if q > 1.0 else q


def run_test(pats, weights, k, x, y, S, rule=0):
    """(G, df, p, N) of one test with libm."""
    N = counts(pats, weights, k, x, y, S)
    g, df = g2(N), df_of(N, rule)
    return g, df, chisq_sf(g, df), N


def tail_close(p, want, tol=CHISQ_TOL) -> bool:
    """p against a reference value of the tail: relative where the reference is a normal double well inside the range."""
    if want >= CHISQ_NORMAL:
        return abs(p - want) <= tol * want
    return 0.0 <= p <= CHISQ_NORMAL * (1.0 + tol)


def golden_grid():
    """The (df, G) grid of tests/golden/chisq_sf.json as scripts/make_chisq_golden.py lays it out."""
    grid = []
    for df in (1, 2, 3, 4, 7, 64, 1000, 65536, 1 << 20):
        d = float(df)
        for g in (0.0, 1e-12, 0.5 * d, d - 1.0, d, d + 2.0, 2.0 * d, 10.0 * d, 10.0 * d + 4000.0):
            grid.append((df, g))
    return grid
