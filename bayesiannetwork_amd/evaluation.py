"""Mirror of bn::evaluation (reference bayesian/evaluation/transinformation.hpp): entropy and mutual
information of the columns of a sample table, on the GPU (bn_info_* of include/bn_mi355x.h).

`InfoTable` holds one table on the device (uploaded and transposed once); `entropy`,
`mutual_information` and `mutual_information_matrix` take either an InfoTable or an `engine.Sampler`,
whose table is keyed by full-node pattern tuples.  For a Sampler only the requested columns are
marshalled; a column's arity is `k[v]` when `k` is given, else its largest sampled state + 1 (the value
of H does not depend on states no sample has).  An empty sampler gives 0.0 without a device call, the
reference's value.  Not in the reference: InfoTable itself and mutual_information_matrix."""
from __future__ import annotations

import ctypes

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
