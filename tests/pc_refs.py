"""Plain Python restatement of bn_learn_pc (include/bn_mi355x.h): the PC-stable skeleton level by level with the lowest-rank
separating set per edge, v-structures, Meek's R1-R3 in the stated scanning order and the Dor-Tarsi extension.  The p-values come
from a callback, so the same loop runs on libm's values (ci_refs) and replays the device's own.  numpy and math only."""
import itertools
import math

import numpy as np

import ci_refs

MAX_NODES, DEFAULT_MAX_TESTS = 1024, 1 << 22


class TooManyTests(Exception):
    pass


def level_tests(k, adj, level):
    """The tests of one level over the adjacency at its start, per edge (a < b) in increasing rank: {(a, b): [(x, y, S), ...]}, the
    over-limit ones included (marked by the caller), and whether any ordered pair qualified."""
    n = len(adj)
    out, any_pair = {}, False
    for a in range(n):
        for b in adj[a]:
            if b < a:
                continue
            seq = []
            for x, y in ((a, b), (b, a)):
                rest = [v for v in adj[x] if v != y]
                if len(rest) >= level:
                    any_pair = True
                    if level == 0 and x > y:
                        continue
                    seq += [(x, y, S) for S in itertools.combinations(rest, level)]
            out[(a, b)] = seq
    return out, any_pair


def cells_of(k, x, y, S) -> int:
    return int(k[x]) * int(k[y]) * math.prod(int(k[v]) for v in S)


def pc_stable(k, p_values, alpha=0.05, max_cond=3, start=None, max_tests=DEFAULT_MAX_TESTS):
    """p_values(tests) -> one p per (x, y, S), called once per level with every test the level runs (rank order within an edge,
    edges in increasing (a, b)).  Returns a dict: skeleton, cpdag [n][n] uint8, sepsets {(a, b): S}, levels [(tests, removed)],
    skipped, margin = the smallest |p - alpha| / alpha over every test visited, visited = the tests per level."""
    n = len(k)
    skel = np.ones((n, n), dtype=np.uint8) - np.eye(n, dtype=np.uint8) if start is None else (np.asarray(start) != 0).astype(np.uint8)
    np.fill_diagonal(skel, 0)
    sepsets, levels, visited, skipped, margin = {}, [], [], 0, math.inf
    for level in range(max_cond + 1):
        adj = [[int(b) for b in np.nonzero(skel[a])[0]] for a in range(n)]
        per_edge, any_pair = level_tests(k, adj, level)
        if not any_pair:
            break
        asked = sum(len(seq) for seq in per_edge.values())
        if asked > max_tests:
            raise TooManyTests(f"level {level} needs {asked} tests")
        run = []
        for edge, seq in per_edge.items():
            for t in seq:
                if cells_of(k, *t) > ci_refs.MAX_CELLS:
                    skipped += 1
                else:
                    run.append((edge, t))
        ps = list(p_values([t for _, t in run])) if run else []
        removed = 0
        for (edge, t), p in zip(run, ps):
            margin = min(margin, abs(p - alpha) / alpha)
            if p > alpha and edge not in sepsets:   # (rank order: the first independent test of the edge is its lowest rank)
                sepsets[edge] = tuple(t[2])
                removed += 1
        for (a, b) in per_edge:
            if (a, b) in sepsets:
                skel[a, b] = skel[b, a] = 0
        levels.append((len(run), removed))
        visited.append([t for _, t in run])
    cpdag = meek(orient_colliders(skel, sepsets))
    return {"skeleton": skel, "cpdag": cpdag, "sepsets": sepsets, "levels": levels, "skipped": skipped, "margin": margin,
            "visited": visited}


def libm_p_values(table, rule=0):
    """The callback on libm: p of every test from ci_refs on a learning_refs.Table."""
    def run(tests):
        return [ci_refs.run_test(table.pats, table.counts, table.k, x, y, S, rule)[2] for x, y, S in tests]
    return run


# ---- orientation ----------------------------------------------------------------------------------

def orient_colliders(skel, sepsets) -> np.ndarray:
    skel = np.asarray(skel, dtype=np.uint8)
    n = skel.shape[0]
    m = skel.copy()
    for z in range(n):
        for x in range(n):
            if x == z or not skel[x, z]:
                continue
            for y in range(x + 1, n):
                if y == z or not skel[y, z] or skel[x, y] or (x, y) not in sepsets or z in sepsets[(x, y)]:
                    continue
                if m[x, z]:
                    m[z, x] = 0
                if m[y, z]:
                    m[z, y] = 0
    return m


def meek(m) -> np.ndarray:
    m = np.array(m, dtype=np.uint8)
    n = m.shape[0]
    und = lambda a, b: m[a, b] and m[b, a]            # noqa: E731
    dire = lambda a, b: m[a, b] and not m[b, a]       # noqa: E731
    adj = lambda a, b: m[a, b] or m[b, a]             # noqa: E731
    changed = True
    while changed:
        changed = False
        for a in range(n):
            for b in range(n):
                if a == b or not und(a, b):
                    continue
                others = [c for c in range(n) if c != a and c != b]
                fire = any(dire(c, a) and not adj(c, b) for c in others)
                fire = fire or any(dire(a, c) and dire(c, b) for c in others)
                fire = fire or any(und(a, c) and dire(c, b) and und(a, d) and dire(d, b) and not adj(c, d)
                                   for c in others for d in others if c < d)
                if fire:
                    m[b, a] = 0
                    changed = True
    return m


def pdag_to_dag(m):
    """Parent lists of the Dor-Tarsi extension (lowest eligible node first), or None where none exists."""
    m = np.array(m, dtype=np.uint8)
    n = m.shape[0]
    np.fill_diagonal(m, 0)
    parents = [[a for a in range(n) if m[a, b] and not m[b, a]] for b in range(n)]
    left = set(range(n))
    while left:
        pick = None
        for x in sorted(left):
            if any(m[x, y] and not m[y, x] for y in left):
                continue
            nbrs = [w for w in left if m[x, w] or m[w, x]]
            if all(m[y, w] or m[w, y] for y in nbrs if m[x, y] and m[y, x] for w in nbrs if w != y):
                pick = x
                break
        if pick is None:
            return None
        parents[pick] += [y for y in left if m[pick, y] and m[y, pick]]
        left.remove(pick)
    return [sorted(p) for p in parents]


def marks(n, directed=(), undirected=()) -> np.ndarray:
    m = np.zeros((n, n), dtype=np.uint8)
    for a, b in directed:
        m[a, b] = 1
    for a, b in undirected:
        m[a, b] = m[b, a] = 1
    return m


# ---- the inputs the CPU test checks and the GPU test relies on ---------------------------------------

ALPHA = 0.05
INPUT_NAMES = ("collider", "chain", "collider_tail", "diamond", "dag12", "alarm")
_NEAR, _FAR = [0.85, 0.15, 0.15, 0.85], [0.5, 0.5]
_BOTH = [0.95, 0.05, 0.4, 0.6, 0.3, 0.7, 0.05, 0.95]            # P(z | x, y): each parent matters, alone and given the other
# name: (parent lists, CPTs, directed edges and undirected edges of the true CPDAG, draws, seed, max_cond); all binary
_SMALL = {
    "collider": ([[], [], [0, 1]], [_FAR, _FAR, _BOTH], [(0, 2), (1, 2)], [], 3000, 1, 3),
    "chain": ([[], [0], [1]], [_FAR, _NEAR, _NEAR], [], [(0, 1), (1, 2)], 3000, 2, 3),
    "collider_tail": ([[], [], [0, 1], [2]], [_FAR, _FAR, _BOTH, _NEAR], [(0, 2), (1, 2), (2, 3)], [], 3000, 3, 3),
    "diamond": ([[], [0], [0], [1, 2]], [_FAR, _NEAR, _NEAR, _BOTH], [(1, 3), (2, 3)], [(0, 1), (0, 2)], 4000, 4, 3),
}
_INPUTS = {}


def pc_input(name):
    """(Table, true CPDAG marks or None, max_cond) of one input of the PC tests; cached per process."""
    import learning_refs as LR
    if name not in _INPUTS:
        if name in _SMALL:
            from bayesiannetwork_amd.flat import from_parent_lists
            parents, cpts, directed, undirected, draws, seed, max_cond = _SMALL[name]
            model = from_parent_lists([2] * len(parents), parents, cpts)
            _INPUTS[name] = (LR.sample_table(model, draws, seed), marks(len(parents), directed, undirected), max_cond)
        elif name == "dag12":
            from bayesiannetwork_amd import synth
            model = synth.random_dag(12, 2, 6, [2, 3, 2, 4], seed=6)
            _INPUTS[name] = (LR.sample_table(model, 3000, 8), None, 3)
        else:
            _INPUTS[name] = (LR.learning_input("alarm2k_mdl")[1], None, 2)
    return _INPUTS[name]


_LIBM = {}


def libm_result(name, rule=0):
    """pc_stable on libm's p-values for an input; cached per process (the GPU tests compare against it)."""
    if (name, rule) not in _LIBM:
        table, _, max_cond = pc_input(name)
        _LIBM[(name, rule)] = pc_stable(table.k, libm_p_values(table, rule), ALPHA, max_cond)
    return _LIBM[(name, rule)]
