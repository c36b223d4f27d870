"""Mirror of bn::evaluation (reference bayesian/evaluation/transinformation.hpp): entropy and mutual
information of the columns of a sample table, on the GPU (bn_info_* of include/bn_mi355x.h).

`InfoTable` holds one table on the device (uploaded and transposed once); `entropy`,
`mutual_information` and `mutual_information_matrix` take either an InfoTable or an `engine.Sampler`,
whose table is keyed by full-node pattern tuples.  For a Sampler only the requested columns are
marshalled; a column's arity is `k[v]` when `k` is given, else its largest sampled state + 1 (the value
of H does not depend on states no sample has).  An empty sampler gives 0.0 without a device call, the
reference's value.  Not in the reference: InfoTable itself and mutual_information_matrix.

Also the mirror of bn::evaluation::aic / mdl (reference bayesian/evaluation/aic.hpp, mdl.hpp over
basic_info_criteria.hpp:44-117): `AIC(sampling)` / `MDL(sampling)` score a network against a table through
bn_score_nodes.  Not in the reference: `log_likelihood_rows` (per distinct pattern), `log_likelihood_nodes`
(per node, optionally with the family counts), `log_cpt` and `parameters` as functions of their own.

`BDeu(ess)` and `K2Score()` are the Bayesian-Dirichlet scores (not in the reference): called on a model and a table they give minus
the log marginal likelihood of the table under the model's structure, the function learning.py's searches minimise under them.

`ci_tests(table, tests)` runs a batch of G^2 conditional-independence tests "x independent of y given S" (bn_ci_tests: the tests of
bnlearn's ci.test "mi" / "mi-adf"; not in the reference) and `chisq_sf(g, df)` evaluates their chi-square tail on the device.

`InfoTable.cond_pair_entropies` / `conditional_mutual_information_matrix` give H(X, Y, Z), H(X, Z), H(Z) and I(X; Y | Z) of every pair
of columns given one conditioning column at once (bn_info_cond_pair_entropies; not in the reference): the weights of learning.TAN."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


class InfoTable:
    """A pattern table on the device: patterns [P][n] states, counts [P] occurrences, k [n] arities."""

    def __init__(self, patterns, counts, k, device: int = _lib.BN_DEVICE_CURRENT):
        k = np.ascontiguousarray(k, dtype=np.int32).reshape(-1)
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, max(len(k), 1))
        counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        if counts.shape[0] != patterns.shape[0]:
            raise ValueError("one count per pattern")
        self.n, self.k = len(k), k
        self.n_patterns, self.total = patterns.shape[0], int(counts.sum(dtype=np.uint64))
        self.device = device
        self.patterns, self.counts = patterns, counts   # (host copies: learning.py fits the learned structure's CPTs to them)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().bn_info_create(patterns.shape[0], len(k), _p(patterns, ctypes.c_uint8),
                                             _p(counts, ctypes.c_uint64), _p(k, ctypes.c_int32), device, ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().bn_info_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def entropy(self, variables, route: int = 0) -> float:
        """Joint entropy (bits) of the columns `variables` (one index or a list); route 0 automatic,
        1 dense cells, 2 sorted packed keys."""
        v = np.ascontiguousarray(np.atleast_1d(variables), dtype=np.int32)
        out = ctypes.c_double()
        _lib.check(_lib.lib().bn_info_entropy(self._h, len(v), _p(v, ctypes.c_int32), route, ctypes.byref(out)))
        return out.value

    def pair_entropies(self, variables=None, mi: bool = True) -> dict:
        """h [m], hxy [m][m] and (mi=True) mi [m][m] = h[x] + h[y] - hxy[x][y] of the columns `variables`
        (None: every column)."""
        if variables is None:
            m, vp = self.n, None
        else:
            v = np.ascontiguousarray(variables, dtype=np.int32).reshape(-1)
            m, vp = len(v), _p(v, ctypes.c_int32)
        h, hxy = np.zeros(m), np.zeros((m, m))
        mim = np.zeros((m, m)) if mi else None
        _lib.check(_lib.lib().bn_info_pair_entropies(self._h, m, vp, _p(h, ctypes.c_double), _p(hxy, ctypes.c_double),
                                                     _p(mim, ctypes.c_double) if mi else None))
        out = {"h": h, "hxy": hxy}
        if mi:
            out["mi"] = mim
        return out

    def pair_counts(self, pairs) -> list:
        """The exact k_x x k_y joint count blocks of `pairs` [(x, y), ...] as the all-pairs kernel made them."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        sizes = [int(self.k[x]) * int(self.k[y]) for x, y in pr]
        out = np.zeros(sum(sizes), dtype=np.uint64)
        _lib.check(_lib.lib().bn_info_pair_counts(self._h, len(pr), _p(pr, ctypes.c_int32), _p(out, ctypes.c_uint64)))
        blocks, o = [], 0
        for (x, y), s in zip(pr, sizes):
            blocks.append(out[o:o + s].reshape(int(self.k[x]), int(self.k[y])))
            o += s
        return blocks

    def cond_pair_entropies(self, cond: int, variables=None, cmi: bool = True) -> dict:
        """hz = H(Z), hxz [m] = H(X, Z), hxyz [m][m] = H(X, Y, Z) and (cmi=True) cmi [m][m] = hxz[x] + hxz[y] - hxyz[x][y] - hz for the
        conditioning column Z = `cond` and the columns `variables` (None: every column but cond)."""
        cond = int(cond)
        if variables is None:
            variables = [v for v in range(self.n) if v != cond]
        v = np.ascontiguousarray(variables, dtype=np.int32).reshape(-1)
        m = len(v)
        hz = ctypes.c_double()
        hxz, hxyz = np.zeros(max(m, 1)), np.zeros((max(m, 1), max(m, 1)))
        cm = np.zeros((max(m, 1), max(m, 1))) if cmi else None
        _lib.check(_lib.lib().bn_info_cond_pair_entropies(self._h, cond, m, _p(v, ctypes.c_int32), ctypes.byref(hz), _p(hxz, ctypes.c_double),
                                                          _p(hxyz, ctypes.c_double), _p(cm, ctypes.c_double) if cmi else None))
        out = {"hz": hz.value, "hxz": hxz, "hxyz": hxyz}
        if cmi:
            out["cmi"] = cm
        return out

    def cond_pair_counts(self, cond: int, pairs) -> list:
        """The exact k_cond x k_x x k_y count blocks of `pairs` [(x, y), ...] as the conditional all-pairs kernel made them."""
        cond = int(cond)
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        kz = int(self.k[cond]) if 0 <= cond < self.n else 1   # (out of range: the library says so)
        ok = all(0 <= int(v) < self.n for v in pr.reshape(-1))
        sizes = [kz * int(self.k[x]) * int(self.k[y]) for x, y in pr] if ok else [1]
        out = np.zeros(max(sum(sizes), 1), dtype=np.uint64)
        _lib.check(_lib.lib().bn_info_cond_pair_counts(self._h, cond, len(pr), _p(pr, ctypes.c_int32), _p(out, ctypes.c_uint64)))
        blocks, o = [], 0
        for (x, y), s in zip(pr, sizes):
            blocks.append(out[o:o + s].reshape(kz, int(self.k[x]), int(self.k[y])))
            o += s
        return blocks

    def last_pairs_ms(self) -> float:
        out = ctypes.c_double()
        _lib.check(_lib.lib().bn_info_last_pairs_ms(self._h, ctypes.byref(out)))
        return out.value

    def info(self, name: str) -> int:
        out = ctypes.c_int64()
        _lib.check(_lib.lib().bn_info_get(self._h, name.encode(), ctypes.byref(out)))
        return out.value


def table_from_sampler(sampler, variables, k=None, device: int = _lib.BN_DEVICE_CURRENT) -> InfoTable:
    """An InfoTable of the columns `variables` of a Sampler's table (column i of the result = variables[i])."""
    vs = [int(v) for v in np.atleast_1d(variables)]
    tab = sampler.table()
    if not tab:
        raise ValueError("empty sampler")
    keys = list(tab.keys())
    full = np.array([key if not isinstance(key, bytes) else tuple(key) for key in keys], dtype=np.int64)
    pats = full[:, vs]
    if (pats < 0).any() or (pats > 254).any():
        raise ValueError("states must be in 0..254")
    counts = np.array([tab[key] for key in keys], dtype=np.uint64)
    if k is None:
        kk = pats.max(axis=0) + 1
    else:
        kk = np.asarray([int(k[v]) for v in vs])
    return InfoTable(pats.astype(np.uint8), counts, kk.astype(np.int32), device)


def _columns(vs):
    """Distinct columns of a variable list and the position of each entry among them."""
    uniq = sorted(set(vs))
    return uniq, [uniq.index(v) for v in vs]


def entropy(sampler_or_table, variables, k=None) -> float:
    """entropy::operator()(sampling, variables) / (sampling, variable) (transinformation.hpp:14-49)."""
    if isinstance(sampler_or_table, InfoTable):
        return sampler_or_table.entropy(variables)
    if sampler_or_table.sampling_size() == 0:
        return 0.0
    uniq, pos = _columns([int(v) for v in np.atleast_1d(variables)])
    with table_from_sampler(sampler_or_table, uniq, k) as t:
        return t.entropy(pos)


def mutual_information(sampler_or_table, x, y, x_ent=None, y_ent=None, k=None) -> float:
    """mutual_information::operator() (transinformation.hpp:52-81): x_ent + y_ent - H(x, y), the entropies
    of x and y computed here unless given (the template overload)."""
    if isinstance(sampler_or_table, InfoTable):
        t = sampler_or_table
        hx = t.entropy(x) if x_ent is None else x_ent
        hy = t.entropy(y) if y_ent is None else y_ent
        return hx + hy - t.entropy([x, y])
    if sampler_or_table.sampling_size() == 0:
        return (0.0 if x_ent is None else x_ent) + (0.0 if y_ent is None else y_ent) - 0.0
    uniq, (px, py) = _columns([int(x), int(y)])
    with table_from_sampler(sampler_or_table, uniq, k) as t:
        hx = t.entropy(px) if x_ent is None else x_ent
        hy = t.entropy(py) if y_ent is None else y_ent
        return hx + hy - t.entropy([px, py])


def mutual_information_from(x_ent, y_ent, xy_ent):
    """The three-entropy overload (transinformation.hpp:77-81)."""
    return x_ent + y_ent - xy_ent


def mutual_information_matrix(sampler_or_table, variables=None, k=None) -> dict:
    """Not in the reference: h [m], hxy [m][m] and mi [m][m] of every pair of `variables` at once (None:
    every column of an InfoTable, every node of a Sampler's patterns)."""
    if isinstance(sampler_or_table, InfoTable):
        return sampler_or_table.pair_entropies(variables)
    if variables is None:
        variables = range(len(next(iter(sampler_or_table.table()))) if sampler_or_table.sampling_size() else 0)
    vs = [int(v) for v in variables]
    if sampler_or_table.sampling_size() == 0:
        m = len(vs)
        return {"h": np.zeros(m), "hxy": np.zeros((m, m)), "mi": np.zeros((m, m))}
    uniq, pos = _columns(vs)
    with table_from_sampler(sampler_or_table, uniq, k) as t:
        return t.pair_entropies(pos)


def conditional_mutual_information_matrix(sampler_or_table, cond, variables=None, k=None) -> dict:
    """Not in the reference: hz, hxz [m], hxyz [m][m] and cmi [m][m] = I(X; Y | cond) of every pair of `variables` at once (None: every
    column of an InfoTable, every node of a Sampler's patterns, but `cond`)."""
    if isinstance(sampler_or_table, InfoTable):
        return sampler_or_table.cond_pair_entropies(cond, variables)
    cond = int(cond)
    if variables is None:
        width = len(next(iter(sampler_or_table.table()))) if sampler_or_table.sampling_size() else 0
        variables = [v for v in range(width) if v != cond]
    vs = [int(v) for v in variables]
    if cond in vs:
        raise ValueError("the conditioning column is among the variables")
    if sampler_or_table.sampling_size() == 0:
        m = len(vs)
        return {"hz": 0.0, "hxz": np.zeros(m), "hxyz": np.zeros((m, m)), "cmi": np.zeros((m, m))}
    uniq, pos = _columns(vs + [cond])
    with table_from_sampler(sampler_or_table, uniq, k) as t:
        return t.cond_pair_entropies(pos[-1], pos[:-1])


# ---- log-likelihood, AIC, MDL (bn_score_* of include/bn_mi355x.h) ---------------------------------

def log_cpt(engine) -> np.ndarray:
    """L[q] = log(cpt[q]) as the engine holds it (fp64 libm log on the host; -inf where the CPT has 0)."""
    out = np.zeros(int(engine.model.cpt_off[-1]))
    _lib.check(_lib.lib().bn_score_log_cpt(engine._h, _p(out, ctypes.c_double)))
    return out


def log_likelihood_rows(engine, table: InfoTable, nodes=None) -> np.ndarray:
    """Per distinct pattern of `table`: the sum over `nodes` (None: every node; any order, no duplicates) of
    log P(state | parents' states) under the engine's network.  The order of additions is the header's, so
    the value of a pattern depends on the model, the selection and that pattern only."""
    out = np.zeros(table.n_patterns)
    if nodes is None:
        m, vp = 0, None
    else:
        v = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        m, vp = len(v), _p(v, ctypes.c_int32)
    _lib.check(_lib.lib().bn_score_rows(engine._h, table._h, m, vp, _p(out, ctypes.c_double)))
    return out


def log_likelihood_nodes(engine, table: InfoTable, counts: bool = False):
    """Per node v: sum over its CPT entries q seen in the table of N[q] * log(cpt[q]) (N: samples showing that
    parent assignment and state).  counts=True: (ll_node, N) with N [n_entries] uint64."""
    out = np.zeros(engine.model.n)
    N = np.zeros(int(engine.model.cpt_off[-1]), dtype=np.uint64) if counts else None
    _lib.check(_lib.lib().bn_score_nodes(engine._h, table._h, _p(out, ctypes.c_double),
                                         _p(N, ctypes.c_uint64) if counts else None))
    return (out, N) if counts else out


def parameters(engine_or_model) -> int:
    """basic_info_criteria::calc_parameters (:100-117): sum over the nodes of (k - 1) x product of the parents' arities."""
    if hasattr(engine_or_model, "_h"):
        return engine_or_model.info("parameters")
    m = engine_or_model
    return sum((int(m.k[v]) - 1) * math.prod(int(m.k[u]) for u in m.parents(v)) for v in range(m.n))


class _InfoCriterion:
    """basic_info_criteria (basic_info_criteria.hpp:13-42): `sampling` is an InfoTable over every node in node
    order, or an engine.Sampler (marshalled at the first call, over all nodes in node order, arities from the
    model, and kept: a sampler reloaded afterwards needs a new functor)."""

    def __init__(self, sampling, device: int = _lib.BN_DEVICE_CURRENT):
        self._sampling, self._device = sampling, device
        self._table = sampling if isinstance(sampling, InfoTable) else None

    def sampling_size(self) -> int:
        return self._sampling.total if isinstance(self._sampling, InfoTable) else self._sampling.sampling_size()

    def _ensure_table(self, model) -> InfoTable:
        if self._table is None:
            self._table = table_from_sampler(self._sampling, range(model.n), model.k, self._device)
        return self._table

    def calc_likelihood(self, engine_or_model, nodes=None) -> float:
        """-log P(D | network) over `nodes` in the given order (:44-78): likelihood = 0.0; likelihood -= ll_node[v]."""
        if self.sampling_size() == 0:   # an empty table: no statistics, no term (the reference's loops run zero times)
            return 0.0
        if hasattr(engine_or_model, "_h"):
            ll = log_likelihood_nodes(engine_or_model, self._ensure_table(engine_or_model.model))
        else:
            from .engine import Engine
            table = self._ensure_table(engine_or_model)
            with Engine(engine_or_model, device=table.device) as eng:
                ll = log_likelihood_nodes(eng, table)
        likelihood = 0.0
        for v in (range(len(ll)) if nodes is None else nodes):
            likelihood -= float(ll[int(v)])
        return likelihood

    def _terms(self, engine_or_model, nodes):
        # parameters: ALWAYS over the whole graph, also for a node subset (aic.hpp:23-24, mdl.hpp:24-25)
        return self.calc_likelihood(engine_or_model, nodes), float(parameters(engine_or_model))


class AIC(_InfoCriterion):
    """bn::evaluation::aic (aic.hpp): score(engine_or_model, nodes=None) = likelihood + parameters."""

    def __call__(self, engine_or_model, nodes=None) -> float:
        likelihood, params = self._terms(engine_or_model, nodes)
        return likelihood + params


class MDL(_InfoCriterion):
    """bn::evaluation::mdl (mdl.hpp): likelihood + parameters * (log2(N) / 2), N the table's total count; an empty
    sampling raises RuntimeError("Sampling is not finished yet.") (:28-36)."""

    def __call__(self, engine_or_model, nodes=None) -> float:
        if self.sampling_size() == 0:
            raise RuntimeError("Sampling is not finished yet.")
        likelihood, params = self._terms(engine_or_model, nodes)
        return likelihood + params * (math.log2(float(self.sampling_size())) / 2)


# ---- Bayesian-Dirichlet scores (bn_score_spec of include/bn_mi355x.h) -------------------------------

class _BDScore:
    """score(model, sampling): minus the log marginal likelihood of `sampling` (an InfoTable over every node in node order, or an
    engine.Sampler) under the structure of `model` (a FlatModel, or per-node parent lists with an InfoTable); the CPTs are not
    read.  Smaller is better.  Computed by the library's learner (bn_learn_create_spec): the bits of `Learner.score()`."""

    kind, ess = 0, 0.0

    def __call__(self, model, sampling) -> float:
        from .learning import Learner
        if isinstance(sampling, InfoTable):
            with Learner(sampling, model, self) as L:
                return L.score()
        with table_from_sampler(sampling, range(model.n), model.k) as t, Learner(t, model, self) as L:
            return L.score()


class BDeu(_BDScore):
    """BDeu with the equivalent sample size `ess` (finite, within [2^-20, 2^20])."""

    kind = 2

    def __init__(self, ess: float = 1.0):
        ess = float(ess)
        if not (math.isfinite(ess) and 2.0 ** -20 <= ess <= 2.0 ** 20):
            raise ValueError(f"BDeu: ess must be finite and within [2^-20, 2^20], not {ess!r}")
        self.ess = ess

    def __repr__(self):
        return f"BDeu(ess={self.ess!r})"


class K2Score(_BDScore):
    """The K2 (Cooper-Herskovits) score: a uniform Dirichlet prior, every hyperparameter 1."""

    kind = 3

    def __repr__(self):
        return "K2Score()"


# ---- conditional-independence tests (bn_ci_tests, bn_ci_chisq_sf) ----------------------------------

DF_RULES = {"nominal": 0, "adjusted": 1}


def _df_rule(df_rule) -> int:
    if df_rule in DF_RULES:
        return DF_RULES[df_rule]
    if df_rule in (0, 1):
        return int(df_rule)
    raise ValueError('df_rule: "nominal" (bnlearn mi) or "adjusted" (mi-adf)')


def ci_tests(table: InfoTable, tests, df_rule="nominal", counts: bool = False, alpha: float = 0.05) -> dict:
    """tests: [(x, y, S), ...], S any iterable of columns in any order.  Returns {"stat": G [T], "df": int64 [T], "p": [T],
    "independent": bool [T] (p > alpha)}; counts=True adds "counts": per test the uint64 table N[s][b][a] (s over the sorted S,
    b the state of y, a the state of x) of shape (strata, k_y, k_x).  The library groups the tests by (x, S); no result depends on
    their order."""
    tests = [(int(x), int(y), [int(v) for v in s]) for x, y, s in tests]
    T = len(tests)
    xs = np.array([t[0] for t in tests], dtype=np.int32)
    ys = np.array([t[1] for t in tests], dtype=np.int32)
    sptr = np.zeros(T + 1, dtype=np.int32)
    for i, t in enumerate(tests):
        sptr[i + 1] = sptr[i] + len(t[2])
    sidx = np.array([v for t in tests for v in t[2]], dtype=np.int32)
    stat, p = np.zeros(max(T, 1)), np.zeros(max(T, 1))
    df, ind = np.zeros(max(T, 1), dtype=np.int64), np.zeros(max(T, 1), dtype=np.uint8)
    N, shapes = None, []
    if counts:
        k, ok = table.k, True
        for x, y, s in tests:
            if not all(0 <= v < table.n for v in [x, y] + s):
                ok = False   # (out of range: the library names the test)
                break
            shapes.append((math.prod(int(k[v]) for v in set(s)), int(k[y]), int(k[x])))
        N = np.zeros(max(sum(a * b * c for a, b, c in shapes) if ok else 1, 1), dtype=np.uint64)
    _lib.check(_lib.lib().bn_ci_tests(table._h, T, _p(xs, ctypes.c_int32), _p(ys, ctypes.c_int32), _p(sptr, ctypes.c_int32),
                                      _p(sidx, ctypes.c_int32), _df_rule(df_rule), float(alpha), _p(stat, ctypes.c_double),
                                      _p(df, ctypes.c_int64), _p(p, ctypes.c_double), _p(ind, ctypes.c_uint8),
                                      _p(N, ctypes.c_uint64) if counts else None))
    out = {"stat": stat[:T], "df": df[:T], "p": p[:T], "independent": ind[:T].astype(bool)}
    if counts:
        blocks, at = [], 0
        for shape in shapes:
            size = shape[0] * shape[1] * shape[2]
            blocks.append(N[at:at + size].reshape(shape))
            at += size
        out["counts"] = blocks
    return out


def chisq_sf(g, df) -> np.ndarray:
    """The chi-square upper tail Q(df / 2, g / 2) as the header states it, evaluated on the current device (bn_ci_chisq_sf)."""
    g = np.ascontiguousarray(np.atleast_1d(g), dtype=np.float64)
    df = np.ascontiguousarray(np.atleast_1d(df), dtype=np.int64)
    if g.shape != df.shape:
        raise ValueError("one df per g")
    out = np.zeros(max(g.size, 1))
    _lib.check(_lib.lib().bn_ci_chisq_sf(g.size, _p(g, ctypes.c_double), _p(df, ctypes.c_int64), _p(out, ctypes.c_double)))
    return out[:g.size]
