"""The first-sweep image of the resident path (option "memo0"; bn_kernels.hip memo0_node, bn_engine_memo.cpp): sweep 0 of a run
reads no message, so the engine keeps what it leaves behind -- built once per CPT image, patched by the launch that applies an
evidence set -- and a run of the grid-barrier form starts at sweep 1.  Everything the caller sees must stay what it was: sweep
count (sweep 0 included), the whole residual history (entry 0 included), beliefs and final messages, bit for bit against the oracle,
NaNs included.  Each case runs on ONE engine, so that the image carries the history of the sets applied before: a node that gets
evidence, changes its state, or loses it again must have its slots recomputed, and only its own.  Shapes (tests/
test_resident_start_gpu.py): a 20 x 30 grid of k = 4 (more than one block, a partly filled tile, root / one-parent / two-parent
tiles) at eight waves per block and at the default, an 8 x 8 grid (one block), k = 2 and 3, and a DAG with more than two children
per node (the all-shapes instantiation)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _resident_tiles(monkeypatch):
    monkeypatch.setenv("BN_DAG", "0")   # k = 4 networks would take the register-resident DAG path by default
    monkeypatch.delenv("BN_MEMO0", raising=False)
    monkeypatch.delenv("BN_RESIDENT_WAVES", raising=False)


@pytest.fixture(scope="module")
def Engine(bnlib):
    from bayesiannetwork_amd.engine import Engine
    return Engine


@pytest.fixture(scope="module")
def grid20x30():
    from bayesiannetwork_amd import synth
    return synth.grid(20, 30, 4, seed=2030)


def _force_resident(eng):
    eng.set_option("small", 0)
    eng.set_option("mid", 0)
    eng.set_option("multisweep", 2)
    eng.set_option("flow", 0)      # the image serves the grid-barrier form
    eng.set_option("direct", 1)
    assert eng.info("resident_eligible") == 1


def _check(eng, oracle_mod, g, ev, eps, max_sweeps=0, memo=1, launches=1, tag=""):
    """One run against the oracle: sweeps, residual history, beliefs, final messages; memo: sweeps the run must have taken from the
    image (None: whatever the constant part of sweep 0's residual allows -- but none when the oracle's run ends with sweep 0)."""
    o = oracle_mod.bp_run(g, ev, eps, max_sweeps, dump_msgs=True)
    r = eng.bp_run(ev, eps, max_sweeps)
    st = eng.bp_stats()
    assert eng.last_path() == 2 and st["sweep_launches"] == launches, tag
    if memo is None:
        assert st["memo_sweeps"] in (0, 1) and (o["sweeps"] > 1 or st["memo_sweeps"] == 0), tag
    else:
        assert st["memo_sweeps"] == memo, tag
    assert r["sweeps"] == o["sweeps"], tag
    assert np.array_equal(eng.bp_residuals(), o["residuals"]), tag
    assert np.array_equal(r["beliefs"], o["beliefs"], equal_nan=True), tag
    pi, lam = eng.bp_messages()
    assert np.array_equal(pi, o["pi_msg"], equal_nan=True) and np.array_equal(lam, o["lambda_msg"], equal_nan=True), tag
    assert st["resident_aborts"] == 0, tag
    return o


def _edge_nodes(eng, g):
    """(parent, child) inside one tile and (parent, child) across a tile boundary, neither touching node 0."""
    tiles = eng.node_tiles()
    same = cross = None
    for v in range(1, g.n):
        for j in range(g.in_ptr[v], g.in_ptr[v + 1]):
            u = int(g.in_idx[j])
            if u == 0:
                continue
            if tiles[u] == tiles[v] and same is None:
                same = (u, v)
            if tiles[u] != tiles[v] and cross is None and (same is None or not {u, v} & set(same)):
                cross = (u, v)
    assert same and cross
    return same, cross


def _node_of_partial_tile(eng, avoid=()):
    tiles = eng.node_tiles()
    count = np.bincount(tiles)
    partial = [t for t in range(count.shape[0]) if 0 < count[t] < 64 and t != tiles[0]]
    assert partial, "the network should have a partly filled tile"
    return next(int(v) for v in np.flatnonzero(tiles == partial[-1])[::-1] if int(v) not in avoid)


def _evidence_sets(eng, g):
    """none, A, B (shares nodes of A -- one of them in another state -- and drops others), none, soft, an all-zero vector, A again.
    A holds the root, a childless node (the last one), a node of the partly filled tile, two neighbours inside one tile and two
    across a tile boundary."""
    from bayesiannetwork_amd import Evidence
    k = int(g.k[0])
    (us, vs), (uc, vc) = _edge_nodes(eng, g)
    last = g.n - 1
    assert not (np.asarray(g.in_idx) == last).any(), "the last node should have no children"
    part = _node_of_partial_tile(eng, avoid={us, vs, uc, vc, last, 0})
    other = next(v for v in range(g.n // 3, g.n) if v not in {us, vs, uc, vc, last, part})
    A = {0: k - 1, last: 0, part: 1, us: k - 1, vs: 0, uc: 1, vc: k - 1}
    B = {0: 0, part: 1, uc: 1, other: k - 1}       # the root in another state, two kept as they were, one new; four dropped
    u = np.full(k, 1.0 / k)
    ramp = np.arange(1, k + 1) / float(np.arange(1, k + 1).sum())
    gap = np.array([0.5] + [0.0] * (k - 2) + [0.5])
    soft = {0: ramp, vs: gap, other: u, last: ramp[::-1].copy()}
    zero = {part: np.zeros(k), vc: k - 1}
    mk = lambda d: Evidence.from_dict(g, d)
    return [("none", None), ("A", mk(A)), ("B", mk(B)), ("none again", None), ("soft", mk(soft)), ("zero", mk(zero)), ("A again", mk(A))]


def _run_sequence(eng, oracle_mod, g, eps=1e-6):
    for name, ev in _evidence_sets(eng, g):
        cap = 6 if name == "zero" else 0   # (NaNs never settle)
        _check(eng, oracle_mod, g, ev, eps, cap, tag=name)
    assert eng.info("memo0_active") == 1


@pytest.mark.parametrize("waves", ["8", "default"])
def test_evidence_sequence_on_one_engine_20x30(Engine, oracle_mod, grid20x30, monkeypatch, waves):
    g = grid20x30
    if waves == "8":
        monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    with Engine(g) as eng:
        _force_resident(eng)
        assert eng.info("resident_blocks") > 1 and (waves != "8" or eng.info("resident_waves") == 8)
        assert eng.info("memo0_active") == 0    # built by the first run that can use it
        _run_sequence(eng, oracle_mod, g)
        sets = dict(_evidence_sets(eng, g))
        # the service-block barrier reads the same image
        eng.set_option("direct", 0)
        _check(eng, oracle_mod, g, sets["B"], 1e-6, tag="direct 0")
        _check(eng, oracle_mod, g, sets["soft"], 1e-6, tag="direct 0 soft")
        eng.set_option("direct", 1)
        # max_sweeps 1: sweep 0 is executed; 2: the image plus one sweep -- messages and res_hist[0..1] show the image itself
        _check(eng, oracle_mod, g, sets["A"], 1e-12, 1, memo=0, tag="cap 1")
        o = _check(eng, oracle_mod, g, sets["A"], 1e-12, 2, tag="cap 2")
        assert o["sweeps"] == 2
        _check(eng, oracle_mod, g, sets["zero"], 1e-12, 2, tag="cap 2 zero")
        _check(eng, oracle_mod, g, None, 1e-12, 2, tag="cap 2 none")
        # eps above what sweep 0 can leave: it has to be executed to know; 0.9 as the constant part allows
        _check(eng, oracle_mod, g, sets["B"], 0.9, memo=None, tag="eps 0.9")
        _check(eng, oracle_mod, g, sets["B"], 1.5, memo=0, tag="eps 1.5")
        _check(eng, oracle_mod, g, sets["B"], 1e-6, tag="eps 1e-6")
        # the option: same bits, and the stats say which ran
        eng.set_option("memo0", 0)
        assert eng.info("memo0_active") == 0
        _check(eng, oracle_mod, g, sets["soft"], 1e-6, memo=0, tag="memo0 0")
        _check(eng, oracle_mod, g, sets["A"], 1e-6, memo=0, tag="memo0 0 A")
        eng.set_option("memo0", 1)
        _check(eng, oracle_mod, g, sets["A"], 1e-6, tag="memo0 1")   # (the image was kept right while the option was off)
        _check(eng, oracle_mod, g, None, 1e-6, tag="memo0 1 none")


def test_evidence_sequence_one_block(Engine, oracle_mod, monkeypatch):
    from bayesiannetwork_amd import Evidence, synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = synth.grid(8, 8, 4, seed=88)
    evA, evB = synth.random_evidence(g, 0.1, seed=1), synth.random_evidence(g, 0.1, seed=2)
    with Engine(g) as eng:
        _force_resident(eng)
        assert eng.info("resident_blocks") == 1
        for name, ev in (("none", None), ("A", evA), ("B", evB), ("root + last", Evidence.from_dict(g, {0: 1, 63: 2})), ("none again", None),
                         ("zero", Evidence.from_dict(g, {9: np.zeros(4)})), ("A again", evA)):
            _check(eng, oracle_mod, g, ev, 1e-6, 6 if name == "zero" else 0, tag=name)
        _check(eng, oracle_mod, g, evA, 1e-12, 1, memo=0)
        _check(eng, oracle_mod, g, evA, 1e-12, 2)


@pytest.mark.parametrize("k", [2, 3])
def test_evidence_sequence_small_arities(Engine, oracle_mod, monkeypatch, k):
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = synth.grid(20, 30, k, seed=2030 + k)
    with Engine(g) as eng:
        _force_resident(eng)
        _run_sequence(eng, oracle_mod, g)
        sets = dict(_evidence_sets(eng, g))
        _check(eng, oracle_mod, g, sets["soft"], 1e-12, 2, tag="cap 2")


def test_more_than_two_children_per_node(Engine, oracle_mod):
    """A DAG with <= 2 parents and up to 8 children per node, dense layout (tests/test_resident_gpu.py::test_resident_trees_and_dags):
    the all-shapes instantiation, and nodes whose pi-messages go to more than two records."""
    from bayesiannetwork_amd import Evidence, synth
    done = 0
    for seed in range(6):
        k = [4, 3, 2][seed % 3]
        d = synth.random_dag(700, 2, 8, k, seed=40 + seed)
        children = np.bincount(d.in_idx, minlength=d.n)
        with Engine(d, lanes_per_node=2) as eng:
            if eng.info("resident_eligible") != 1 or children.max() <= 2:
                continue
            _force_resident(eng)
            busy = int(np.argmax(children))                    # the node with the most children, and one without any
            leaf = int(np.flatnonzero(children == 0)[-1])
            evs = [None, Evidence.from_dict(d, {busy: 0, leaf: k - 1}), synth.random_evidence(d, 0.03, seed=seed),
                   Evidence.from_dict(d, {busy: np.full(k, 1.0 / k)}), None, Evidence.from_dict(d, {busy: k - 1, leaf: k - 1})]
            for i, ev in enumerate(evs):
                _check(eng, oracle_mod, d, ev, 1e-6, tag=f"seed {seed} set {i}")
            _check(eng, oracle_mod, d, evs[1], 1e-12, 2, tag=f"seed {seed} cap 2")
            done += 1
            if done == 2:
                break
    assert done >= 1


def test_run_of_two_launches(Engine, oracle_mod, grid20x30, monkeypatch):
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    ev = synth.random_evidence(g, 0.02, seed=5)
    with Engine(g) as eng:
        _force_resident(eng)
        for _ in range(2):
            o = _check(eng, oracle_mod, g, ev, 0.0, 1030, launches=2)
            assert o["sweeps"] == 1030


def test_reload_cpt_rebuilds_the_image(Engine, oracle_mod, grid20x30, monkeypatch):
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    g2 = synth.grid(20, 30, 4, seed=77)    # the same structure, other tables
    assert np.array_equal(g.in_idx, g2.in_idx) and not np.array_equal(g.cpt, g2.cpt)
    ev = synth.random_evidence(g, 0.03, seed=8)
    with Engine(g) as eng:
        _force_resident(eng)
        _check(eng, oracle_mod, g, ev, 1e-6)
        assert eng.info("memo0_active") == 1
        eng.reload_cpt(g2.cpt)
        assert eng.info("memo0_active") == 0
        _check(eng, oracle_mod, g2, ev, 1e-6, tag="new tables")
        assert eng.info("memo0_active") == 1
        _check(eng, oracle_mod, g2, None, 1e-6, tag="new tables, none")
        _check(eng, oracle_mod, g2, ev, 1e-12, 2, tag="new tables, cap 2")


def test_other_paths_between_runs(Engine, oracle_mod, grid20x30, monkeypatch):
    """Resident path, the same evidence on the per-sweep launches, the resident path again, then a batch of two sets."""
    from bayesiannetwork_amd import Evidence, synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    ev = synth.random_evidence(g, 0.03, seed=9)
    evs = [synth.random_evidence(g, 0.05, seed=6), Evidence.from_dict(g, {0: 3, 599: 0})]
    with Engine(g) as eng:
        _force_resident(eng)
        o = _check(eng, oracle_mod, g, ev, 1e-6)
        eng.set_option("multisweep", 0)
        r = eng.bp_run(ev, 1e-6)
        assert eng.last_path() == 0 and eng.bp_stats()["memo_sweeps"] == 0
        assert r["sweeps"] == o["sweeps"] and np.array_equal(r["beliefs"], o["beliefs"]) and np.array_equal(eng.bp_residuals(), o["residuals"])
        eng.set_option("multisweep", 2)
        _check(eng, oracle_mod, g, ev, 1e-6, tag="resident again")
        want = [oracle_mod.bp_run(g, e, 1e-6) for e in evs]
        out = eng.bp_run_batch(evs, 1e-6)
        assert eng.last_path() == 2 and eng.bp_stats()["memo_sweeps"] == 0
        for q, w in enumerate(want):
            assert out["sweeps"][q] == w["sweeps"], f"set {q}"
            assert np.array_equal(out["beliefs"][q], w["beliefs"]), f"set {q}"
            assert np.array_equal(eng.bp_residuals_batch(q), w["residuals"]), f"set {q}"
        _check(eng, oracle_mod, g, ev, 1e-6, tag="after the batch")
        for e, w in zip(evs, want):
            _check(eng, oracle_mod, g, e, 1e-6, tag="a set of the batch alone")
        assert eng.bp_stats()["resident_aborts"] == 0
