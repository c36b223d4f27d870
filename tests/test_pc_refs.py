"""The host restatement of PC-stable (tests/pc_refs.py) on its own: it recovers the true CPDAG of four small networks from sampled
tables, its decisions on every input the GPU tests use are far from the threshold, and the orientation rules and the DAG extension
do what the header states on hand-built graphs."""
import numpy as np
import pytest

import ci_refs as C
import pc_refs as P

# every decision p > alpha of the inputs must sit at least this far (relative to alpha) from the threshold: 100 times the
# tolerance asserted on the device's p-values, so a device p within tolerance decides as libm's does
MARGIN = 100 * C.CHISQ_TOL


@pytest.mark.parametrize("name", ["collider", "chain", "collider_tail", "diamond"])
def test_recovers_the_true_cpdag(name):
    table, true, _ = P.pc_input(name)
    r = P.libm_result(name)
    assert np.array_equal(r["cpdag"], true), (r["cpdag"], r["sepsets"])
    assert np.array_equal(r["skeleton"], ((true + true.T) > 0).astype(np.uint8))
    if name == "collider":
        assert r["sepsets"] == {(0, 1): ()} and len(r["levels"]) == 2            # x -> z <- y, oriented at level 0's sepset
    if name == "chain":
        assert r["sepsets"] == {(0, 2): (1,)} and not (r["cpdag"] != r["cpdag"].T).any()   # a _||_ c | b, nothing oriented
    if name == "collider_tail":
        assert r["cpdag"][2, 3] == 1 and r["cpdag"][3, 2] == 0                   # R1: z -> w
    if name == "diamond":
        assert r["sepsets"] == {(1, 2): (0,), (0, 3): (1, 2)}                    # levels 1 and 2
        assert [lv[1] for lv in r["levels"]] == [0, 1, 1]


@pytest.mark.parametrize("name", P.INPUT_NAMES)
@pytest.mark.parametrize("rule", [0, 1])
def test_margins_of_the_gpu_inputs(name, rule):
    r = P.libm_result(name, rule)
    print(f"{name} rule {rule}: smallest |p - alpha| / alpha = {r['margin']:.3e} over {sum(t for t, _ in r['levels'])} tests")
    # measured: 1.0 on the four small networks (the nearest p is 0), 1.2e-1 on dag12, 3.0e-2 on the ALARM-shaped table
    assert r["margin"] > MARGIN and r["skipped"] == 0


def test_meek_r2_r3_and_first_wins():
    # R2: a -> c -> b with a - b gives a -> b
    m = P.meek(P.marks(3, directed=[(0, 2), (2, 1)], undirected=[(0, 1)]))
    assert m[0, 1] == 1 and m[1, 0] == 0
    # R3: a - c, a - d, c -> b <- d, c and d not adjacent, a - b gives a -> b   (a 0, b 1, c 2, d 3)
    m = P.meek(P.marks(4, directed=[(2, 1), (3, 1)], undirected=[(0, 2), (0, 3), (0, 1)]))
    assert m[0, 1] == 1 and m[1, 0] == 0 and m[0, 2] == m[2, 0] == 1 and m[0, 3] == m[3, 0] == 1
    # no rule: a triangle stays undirected
    tri = P.marks(3, undirected=[(0, 1), (0, 2), (1, 2)])
    assert np.array_equal(P.meek(tri), tri)
    # first wins: the triples (z 1: 0, 2) and (z 2: 1, 3) both claim the edge 1 - 2; z = 1 comes first, so 2 -> 1 stays
    skel = P.marks(4, undirected=[(0, 1), (1, 2), (2, 3)])
    m = P.orient_colliders(skel, {(0, 2): (), (1, 3): (), (0, 3): ()})
    assert m[0, 1] == 1 and m[1, 0] == 0 and m[2, 1] == 1 and m[1, 2] == 0
    assert m[3, 2] == 1 and m[2, 3] == 0            # 3 -> 2 is oriented; 1 -> 2 is not (it is 2 -> 1 already)
    # a pair with no recorded sepset makes no v-structure
    assert np.array_equal(P.orient_colliders(P.marks(3, undirected=[(0, 2), (1, 2)]), {}), P.marks(3, undirected=[(0, 2), (1, 2)]))


def acyclic(parents):
    seen, state = set(), {}

    def visit(v):
        if state.get(v) == 1:
            return False
        if v in seen:
            return True
        state[v] = 1
        ok = all(visit(u) for u in parents[v])
        state[v] = 2
        seen.add(v)
        return ok
    return all(visit(v) for v in range(len(parents)))


def test_dor_tarsi():
    # a chain 0 - 1 - 2: an extension without a new v-structure
    par = P.pdag_to_dag(P.marks(3, undirected=[(0, 1), (1, 2)]))
    assert par == [[1], [2], []]            # the lowest eligible node first: 0 takes 1 -> 0, then 1 takes 2 -> 1
    # directed edges are kept, the undirected one oriented without a cycle
    par = P.pdag_to_dag(P.marks(4, directed=[(0, 2), (1, 2)], undirected=[(2, 3)]))
    assert par == [[], [], [0, 1], [2]]
    # the diamond's CPDAG
    par = P.pdag_to_dag(P.pc_input("diamond")[1])
    assert acyclic(par) and par[3] == [1, 2] and {(u, v) for v, ps in enumerate(par) for u in ps} >= {(1, 3), (2, 3)}
    # an undirected four-cycle has no extension without a new v-structure; nor has a directed cycle
    assert P.pdag_to_dag(P.marks(4, undirected=[(0, 1), (1, 2), (2, 3), (3, 0)])) is None
    assert P.pdag_to_dag(P.marks(3, directed=[(0, 1), (1, 2), (2, 0)])) is None


def test_start_adjacency_and_test_cap():
    table, _, _ = P.pc_input("diamond")
    start = P.marks(4, undirected=[(0, 1), (0, 2), (1, 3), (2, 3)])
    r = P.pc_stable(table.k, P.libm_p_values(table), P.ALPHA, 3, start=start)
    assert np.array_equal(r["skeleton"], start) and r["sepsets"] == {} and r["levels"][0][0] == 4
    with pytest.raises(P.TooManyTests):
        P.pc_stable(table.k, P.libm_p_values(table), P.ALPHA, 3, max_tests=5)
