"""bn_learn_pc on the device against the host restatement (tests/pc_refs.py): replayed with the device's own p-values the restatement
gives exactly the device's skeleton, separating sets, CPDAG and per-level counts; on the margin-checked inputs (tests/test_pc_refs.py)
the result also equals the restatement on libm's p-values, and the true CPDAG of the four small networks."""
import numpy as np
import pytest

import pc_refs as P

pytestmark = pytest.mark.gpu

SMALL = ("collider", "chain", "collider_tail", "diamond")
_TABLES = {}


@pytest.fixture(scope="module")
def tables(bnlib):
    """name -> InfoTable on the device, made on first use and closed with the module."""
    from bayesiannetwork_amd.evaluation import InfoTable

    def get(name):
        if name not in _TABLES:
            t = P.pc_input(name)[0]
            _TABLES[name] = InfoTable(t.pats, t.counts, t.k, device=0)
        return _TABLES[name]
    yield get
    for t in _TABLES.values():
        t.close()
    _TABLES.clear()


def device_p_values(table, rule):
    from bayesiannetwork_amd.evaluation import ci_tests
    return lambda tests: ci_tests(table, tests, df_rule=rule)["p"].tolist()


def same(result, want):
    """A PCResult against a pc_refs result."""
    assert np.array_equal(result.skeleton, want["skeleton"])
    assert result.sepsets == want["sepsets"]
    assert np.array_equal(result.cpdag, want["cpdag"])
    assert [(lv["tests"], lv["removed"]) for lv in result.levels] == want["levels"]
    assert result.tests_skipped == want["skipped"]


@pytest.mark.parametrize("name", P.INPUT_NAMES)
@pytest.mark.parametrize("rule", [0, 1])
def test_replay_and_libm_parity(tables, name, rule):
    from bayesiannetwork_amd.learning import PC
    table, true, max_cond = P.pc_input(name)
    t = tables(name)
    got = PC(P.ALPHA, max_cond, rule)(t)
    same(got, P.pc_stable(table.k, device_p_values(t, rule), P.ALPHA, max_cond))   # the device's own p-values
    same(got, P.libm_result(name, rule))                                          # libm's: the margins are far wider than the tolerance
    if true is not None:
        assert np.array_equal(got.cpdag, true)
    assert all(lv["count_ns"] > 0 and lv["stat_ns"] > 0 for lv in got.levels if lv["tests"])
    assert t.info("ci_stat_ns") > 0


def test_start_adjacency(tables):
    from bayesiannetwork_amd.learning import PC
    table = P.pc_input("dag12")[0]
    rng = np.random.default_rng(4)
    start = np.triu(rng.random((12, 12)) < 0.6, 1).astype(np.uint8)
    start = start + start.T
    got = PC(P.ALPHA, 3)(tables("dag12"), start=start)
    want = P.pc_stable(table.k, P.libm_p_values(table), P.ALPHA, 3, start=start)
    same(got, want)
    assert not (got.skeleton & (1 - start)).any() and all(start[a, b] for a, b in got.sepsets)
    with pytest.raises(Exception, match="not symmetric"):
        PC(P.ALPHA, 3)(tables("dag12"), start=np.triu(start))


def test_several_chunks_per_level_change_nothing(tables, monkeypatch):
    from bayesiannetwork_amd.learning import PC
    t = tables("alarm")
    before = t.info("ci_launches")
    one = PC(P.ALPHA, 2)(t)
    plain = t.info("ci_launches") - before
    monkeypatch.setenv("BN_CI_SCRATCH_CELLS", "2000")
    many = PC(P.ALPHA, 2)(t)
    monkeypatch.delenv("BN_CI_SCRATCH_CELLS")
    assert plain == 2 * len(one.levels) and t.info("ci_launches") - before - plain >= 3 * plain   # several chunks per level
    assert np.array_equal(one.skeleton, many.skeleton) and one.sepsets == many.sepsets and np.array_equal(one.cpdag, many.cpdag)
    assert [(lv["tests"], lv["removed"]) for lv in one.levels] == [(lv["tests"], lv["removed"]) for lv in many.levels]


def test_limits_are_refused(tables, bnlib):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.learning import PC
    t = tables("diamond")
    before = t.info("ci_launches")
    with pytest.raises(_lib.BnError) as e:
        PC(P.ALPHA, 3, max_tests=5)(t)           # level 0 of four nodes asks for six tests
    assert e.value.code == _lib.BN_ERR_STATE and "level 0 needs 6 tests" in str(e.value) and t.info("ci_launches") == before
    with pytest.raises(_lib.BnError) as e:
        PC(P.ALPHA, 3, max_tests=20)(t)          # level 1 asks for 24: refused as a whole, nothing trimmed
    assert e.value.code == _lib.BN_ERR_STATE and "level 1 needs 24 tests" in str(e.value)
    for bad in (dict(alpha=1.0), dict(alpha=0.0), dict(max_cond=9), dict(max_cond=-1)):
        with pytest.raises(_lib.BnError) as e:
            PC(**{"alpha": P.ALPHA, "max_cond": 3, **bad})(t)
        assert e.value.code == _lib.BN_ERR_ARG
    only = PC(P.ALPHA, 0)(t)
    assert [(lv["tests"], lv["removed"]) for lv in only.levels] == [(6, 0)] and only.sepsets == {}


def test_round_trip_into_a_learner(tables):
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.learning import PC, Learner, cpdag_to_dag
    t = tables("alarm")
    r = PC(P.ALPHA, 2)(t)
    parents = cpdag_to_dag(r.cpdag)
    assert parents == P.pdag_to_dag(r.cpdag) == r.dag()
    edges = {(u, v) for v, ps in enumerate(parents) for u in ps}
    assert {(min(e), max(e)) for e in edges} == {(a, b) for a in range(t.n) for b in range(a + 1, t.n) if r.skeleton[a, b]}
    assert all((a, b) in edges for a in range(t.n) for b in range(t.n) if r.cpdag[a, b] and not r.cpdag[b, a])   # directed marks kept
    with Learner(t, structure=parents, criterion="mdl") as L, Learner(t, None, "mdl") as empty:
        assert np.isfinite(L.score()) and L.score() < empty.score()
    with pytest.raises(_lib.BnError) as e:
        cpdag_to_dag(P.marks(4, undirected=[(0, 1), (1, 2), (2, 3), (3, 0)]))
    assert e.value.code == _lib.BN_ERR_STATE
