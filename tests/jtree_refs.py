"""Plain numpy fp64 restatement of junction-tree propagation as include/bn_mi355x.h states it (bn_jt_run), over the plan the library
dumps (Engine.jt_plan()).  It restates the ARITHMETIC -- base potentials, evidence, collect, distribute, read-out, every sum in the
stated order -- with index arithmetic of its own (numpy axes, no item tables); the planner is checked by ``check_plan`` and by
tests/cpp/test_jt_plan.cpp.  The GPU tests compare beliefs and scale arrays with this bit for bit."""
from __future__ import annotations

import numpy as np

from bayesiannetwork_amd import synth

import exact_refs as xr

MIXED = [2, 3, 4]
RUN = 64


def networks():
    """name -> model of every network of the issue's table that the plan takes."""
    return {
        "pearl": synth.pearl(),
        "alarm": alarm(),
        "arity7": synth.random_dag(16, 2, 8, [7, 5, 6, 2], seed=8),
        "grid3x8": synth.grid(3, 8, 4, seed=1),
        "dag37": synth.random_dag(37, 4, 16, MIXED, seed=5),
        "star": xr.star(120, 3, 5),
        "wide12": xr.wide(12),
        "grid8x8k2": synth.grid(8, 8, 2, seed=1),
        "grid4x40": synth.grid(4, 40, 4, seed=1),
        "chain3000": xr.chain(3000, 3),
    }


def alarm():
    import os
    from bayesiannetwork_amd.dsc import load_dsc
    return load_dsc(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alarm_shaped.dsc"))[0]


def hard_evidence(model, frac, seed):
    """About frac * n nodes observed at the states of one forward sample (P(e) > 0)."""
    return xr.draw_evidence(model, max(1, int(round(frac * model.n))), seed=seed)


def ev_state_of(model, ev):
    st = np.full(model.n, -1, dtype=np.int64)
    for j in range(ev.ne):
        st[int(ev.node[j])] = int(np.argmax(ev.val[ev.off[j]:ev.off[j + 1]]))
    return st


# ---- the plan's properties ----------------------------------------------------------------------------------------------------

def check_plan(model, plan):
    nc = plan["cliques"]
    cl = [plan["vars"][plan["var_ptr"][c]:plan["var_ptr"][c + 1]].tolist() for c in range(nc)]
    sp = [plan["sep_vars"][plan["sep_ptr"][c]:plan["sep_ptr"][c + 1]].tolist() for c in range(nc)]
    par, lvl = plan["parent"], plan["level"]
    k = model.k
    assert sorted(plan["order"].tolist()) == list(range(model.n))
    for c in range(nc):
        assert cl[c] == sorted(set(cl[c])) and cl[c], "variables ascending, none twice"
        assert not any(c != d and set(cl[c]) <= set(cl[d]) for d in range(nc) if len(cl[d]) >= len(cl[c])), "maximal cliques only"
        if par[c] < 0:
            assert lvl[c] == 0 and sp[c] == []
        else:
            assert par[c] < c and lvl[c] == lvl[par[c]] + 1, "levels follow parents, a parent has the lower id"
            assert sp[c] == sorted(set(cl[c]) & set(cl[par[c]])) and sp[c], "separator = intersection of the two cliques"
    assert all(lvl[c] <= lvl[c + 1] for c in range(nc - 1)), "numbered level by level"
    assert plan["levels"] == int(lvl.max()) + 1
    # every family inside its clique, every node inside its home
    for v in range(model.n):
        fam = {v, *[int(p) for p in model.parents(v)]}
        assert fam <= set(cl[plan["cpt_clique"][v]])
        assert v in cl[plan["home"][v]]
    # running intersection: the cliques that hold a variable form a connected subtree -- all but one have their parent among them
    for v in range(model.n):
        holds = [c for c in range(nc) if v in cl[c]]
        assert sum(1 for c in holds if par[c] < 0 or v not in cl[par[c]]) == 1
    sizes = [int(np.prod(k[cl[c]], dtype=np.int64)) for c in range(nc)]
    seps = [int(np.prod(k[sp[c]], dtype=np.int64)) for c in range(nc)]
    assert plan["pot_cells"] == sum(sizes) and plan["sep_cells"] == sum(seps) and plan["max_clique"] == max(sizes)
    assert plan["state_cells"] == sum(sizes) + sum(seps) + int(k.sum()) + nc
    return cl, sp


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------

def _two_level(m):
    """m [S, T]: per row the two-level sum of its T terms."""
    total = np.zeros(m.shape[0])
    for r in range(0, m.shape[1], RUN):
        run = np.zeros(m.shape[0])
        for t in range(r, min(r + RUN, m.shape[1])):
            run = run + m[:, t]
        total = total + run
    return total


def _left_to_right(vec):
    s = 0.0
    for x in vec:
        s = s + float(x)
    return s


def _spread(vec, sub, big, k):
    """A table over `sub` as one over `big` (both ascending) with extent 1 on the other axes."""
    return np.asarray(vec).reshape([int(k[u]) if u in sub else 1 for u in big])


def _onto(arr, big, sub, k):
    """The two-level sums of table `arr` over `big` onto `sub`: the terms of one entry in ascending entry index."""
    first = [i for i, u in enumerate(big) if u in sub]
    rest = [i for i, u in enumerate(big) if u not in sub]
    s = int(np.prod([k[big[i]] for i in first], dtype=np.int64)) if first else 1
    return _two_level(np.transpose(arr, first + rest).reshape(s, -1))


class Restatement:
    """The plan as lists, the base potentials of `model`; ``run(evidence)`` -> (beliefs [sum k], scales [cliques], log P(e))."""

    def __init__(self, model, plan):
        self.model, self.plan = model, plan
        nc = plan["cliques"]
        self.k = k = [int(x) for x in model.k]
        self.cl = [plan["vars"][plan["var_ptr"][c]:plan["var_ptr"][c + 1]].tolist() for c in range(nc)]
        self.sp = [plan["sep_vars"][plan["sep_ptr"][c]:plan["sep_ptr"][c + 1]].tolist() for c in range(nc)]
        self.par = plan["parent"].tolist()
        self.kids = [[] for _ in range(nc)]
        for c in range(nc):
            if self.par[c] >= 0:
                self.kids[self.par[c]].append(c)
        lvl = plan["level"]
        self.by_level = [[c for c in range(nc) if lvl[c] == l] for l in range(plan["levels"])]
        self.homed = [[] for _ in range(nc)]
        for v in range(model.n):
            self.homed[plan["home"][v]].append(v)
        self.psi0 = []
        tabs = [[] for _ in range(nc)]
        for v in range(model.n):
            tabs[plan["cpt_clique"][v]].append(v)
        for c in range(nc):
            arr = np.ones([k[u] for u in self.cl[c]])
            for v in tabs[c]:
                fam = [int(p) for p in model.parents(v)] + [v]
                t = np.asarray(model.cpt_of(v), dtype=np.float64).reshape([k[u] for u in fam])
                t = np.transpose(t, np.argsort(fam))   # axes in ascending node id
                arr = arr * _spread(t, set(fam), self.cl[c], k)
            self.psi0.append(arr)

    def run(self, evidence=None):
        k, cl, sp, par = self.k, self.cl, self.sp, self.par
        nc = len(cl)
        ev = {}
        if evidence is not None:
            for j in range(evidence.ne):
                ev[int(evidence.node[j])] = np.asarray(evidence.val[evidence.off[j]:evidence.off[j + 1]], dtype=np.float64)
        pot = []
        for c in range(nc):
            arr = self.psi0[c]
            for v in self.homed[c]:
                if v in ev:
                    arr = arr * _spread(ev[v], {v}, cl[c], k)
            pot.append(arr)
        scales = np.zeros(nc)
        msg = [None] * nc
        with np.errstate(all="ignore"):
            for l in range(len(self.by_level) - 1, -1, -1):
                for c in self.by_level[l]:
                    raw = _onto(pot[c], cl[c], set(sp[c]), k)
                    s = _left_to_right(raw)
                    scales[c] = s
                    msg[c] = raw / s if s > 0 else raw
                if l == 0:
                    break
                for p in self.by_level[l - 1]:
                    for c in self.kids[p]:   # ascending child id
                        pot[p] = pot[p] * _spread(msg[c], set(sp[c]), cl[p], k)
            for l in range(1, len(self.by_level)):
                for c in self.by_level[l]:
                    new = _onto(pot[par[c]], cl[par[c]], set(sp[c]), k)
                    ratio = np.where(msg[c] == 0.0, 0.0, new / msg[c])
                    pot[c] = pot[c] * _spread(ratio, set(sp[c]), cl[c], k)
            out = []
            for v in range(self.model.n):
                h = int(self.plan["home"][v])
                u = _onto(pot[h], cl[h], {v}, k)
                out.append(u / _left_to_right(u))
            lg = 0.0
            for s in scales:
                lg = lg + float(np.log(s))
        return np.concatenate(out), scales, lg


def same_bits(a, b):
    """Equal as bit patterns, NaNs equal to NaNs of any payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
