"""The second-sweep image of the resident path (option "memo1"; bn_kernels.hip memo_step_node, bn_engine_memo.cpp): what sweep 1 of a
run leaves at a node depends on the CPTs and on the evidence of the node's closed neighbourhood alone, so the engine keeps it -- built
once per CPT image, recomputed on the ring around the evidence by a launch behind the one that applies a set -- and a run of the
grid-barrier form starts at sweep 2.  Everything the caller sees must stay what it was: sweep count, the whole residual history
(entries 0 and 1 included), beliefs and final messages, bit for bit against the oracle, NaNs included.  Each case runs on ONE engine,
so that the image carries the history of the sets applied before.  Set-up and shapes as tests/test_resident_memo_gpu.py.  The sets
are staged (bn_bp_set_evidence) unless a case is about the one-shot calls: those decide for themselves whether they patch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _resident_tiles(monkeypatch):
    monkeypatch.setenv("BN_DAG", "0")   # k = 4 networks would take the register-resident DAG path by default
    for name in ("BN_MEMO0", "BN_MEMO1", "BN_MEMO1_LIMIT", "BN_MEMO1_ONESHOT", "BN_RESIDENT_WAVES"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def Engine(bnlib):
    from bayesiannetwork_amd.engine import Engine
    return Engine


@pytest.fixture(scope="module")
def grid20x30():
    from bayesiannetwork_amd import synth
    return synth.grid(20, 30, 4, seed=2030)


_ORACLE = {}


def _oracle(oracle_mod, g, ev, eps, max_sweeps):
    """One oracle run per (network, set, eps, cap), shared by the cases that repeat it."""
    key = (g.name, None if ev is None else (ev.node.tobytes(), ev.val.tobytes()), eps, max_sweeps)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.bp_run(g, ev, eps, max_sweeps, dump_msgs=True)
    return _ORACLE[key]


def _force_resident(eng):
    eng.set_option("small", 0)
    eng.set_option("mid", 0)
    eng.set_option("multisweep", 2)
    eng.set_option("flow", 0)      # the images serve the grid-barrier form
    eng.set_option("direct", 1)
    assert eng.info("resident_eligible") == 1


def _compare(eng, r, beliefs, o, depth, launches, tag):
    st = eng.bp_stats()
    assert eng.last_path() == 2 and st["sweep_launches"] == launches, tag
    assert st["resident_aborts"] == 0, tag
    assert st["memo_depth"] <= max(o["sweeps"] - 1, 0), (tag, st["memo_depth"], o["sweeps"])
    assert st["memo_sweeps"] == (1 if st["memo_depth"] >= 1 else 0), tag
    if isinstance(depth, int):
        assert st["memo_depth"] == depth, (tag, st["memo_depth"])
    else:
        assert st["memo_depth"] in depth, (tag, st["memo_depth"])
    assert r["sweeps"] == o["sweeps"], tag
    assert np.array_equal(eng.bp_residuals(), o["residuals"]), (tag, eng.bp_residuals()[:4], o["residuals"][:4])
    assert np.array_equal(beliefs, o["beliefs"], equal_nan=True), tag
    pi, lam = eng.bp_messages()
    assert np.array_equal(pi, o["pi_msg"], equal_nan=True) and np.array_equal(lam, o["lambda_msg"], equal_nan=True), tag
    return st


def _check(eng, oracle_mod, g, ev, eps, max_sweeps=0, depth=2, launches=1, tag="", stage=True):
    """One run against the oracle.  stage: the set is staged first (bn_bp_set_evidence) and the run uses what is staged; otherwise
    None leaves the staged set alone and runs it again."""
    o = _oracle(oracle_mod, g, ev, eps, max_sweeps)
    if stage:
        eng.bp_set_evidence(ev)
    r = eng.bp_run_device(eps, max_sweeps)
    return _compare(eng, r, eng.bp_beliefs(), o, depth, launches, tag)


def _neighbours(g):
    nb = [set() for _ in range(g.n)]
    for v in range(g.n):
        for j in range(g.in_ptr[v], g.in_ptr[v + 1]):
            u = int(g.in_idx[j])
            nb[v].add(u)
            nb[u].add(v)
    return nb


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
    """none, A, B, none, soft vectors, an all-zero vector, A again.  A holds the root, the childless last node, a node of the partly
    filled tile, two neighbours inside one tile and two across a tile boundary, two nodes (p, q) that share the non-evidence neighbour
    w, and both parents (y0, y1) of the non-evidence node y.  B drops some of A's nodes, keeps some, puts the root into another
    state and adds one; it drops p and keeps q, so w stays in a kept node's ring while it leaves a dropped node's."""
    from bayesiannetwork_amd import Evidence
    k = int(g.k[0])
    nb = _neighbours(g)
    (us, vs), (uc, vc) = _edge_nodes(eng, g)
    last = g.n - 1
    assert not (np.asarray(g.in_idx) == last).any(), "the last node should have no children"
    part = _node_of_partial_tile(eng, avoid={us, vs, uc, vc, last, 0})
    used = {0, last, part, us, vs, uc, vc}
    near = set(used).union(*(nb[v] for v in used))
    # w: no evidence, nowhere near the nodes above; p, q two of its neighbours that are not neighbours of each other
    w, p, q = next((w, a, b) for w in range(g.n // 4, g.n) if w not in near and len(nb[w]) >= 2
                   for a in sorted(nb[w]) for b in sorted(nb[w]) if a < b and a not in near and b not in near and b not in nb[a])
    used |= {p, q}
    near |= {w, p, q} | nb[p] | nb[q] | nb[w]
    # y: no evidence, two parents
    y = next(v for v in range(g.n // 2, g.n) if g.in_ptr[v + 1] - g.in_ptr[v] == 2 and not ({v} | nb[v]) & near)
    y0, y1 = (int(x) for x in g.in_idx[g.in_ptr[y]:g.in_ptr[y + 1]])
    used |= {y0, y1}
    other = next(v for v in range(g.n // 3, g.n) if v not in used and v not in (w, y))
    A = {0: k - 1, last: 0, part: 1, us: k - 1, vs: 0, uc: 1, vc: k - 1, p: 0, q: k - 1, y0: 1, y1: 0}
    assert w not in A and y not in A and {p, q} <= nb[w] and {y0, y1} <= nb[y]
    B = {0: 0, part: 1, uc: 1, q: k - 1, y0: 1, other: k - 1}
    u = np.full(k, 1.0 / k)
    ramp = np.arange(1, k + 1) / float(np.arange(1, k + 1).sum())
    gap = np.array([0.5] + [0.0] * (k - 2) + [0.5])
    soft = {0: ramp, vs: gap, other: u, last: ramp[::-1].copy(), p: gap, y1: ramp}
    zero = {part: np.zeros(k), vc: k - 1}
    mk = lambda d: Evidence.from_dict(g, d)
    return [("none", None), ("A", mk(A)), ("B", mk(B)), ("none again", None), ("soft", mk(soft)), ("zero", mk(zero)), ("A again", mk(A))]


def _run_sequence(eng, oracle_mod, g, eps=1e-6):
    """Every set at eps 1e-6 from sweep 2, then again cut off behind sweep 2: the final messages are then one sweep away from the image."""
    for name, ev in _evidence_sets(eng, g):
        cap = 6 if name == "zero" else 0   # (NaNs never settle)
        _check(eng, oracle_mod, g, ev, eps, cap, tag=name)
        _check(eng, oracle_mod, g, ev, 1e-12, 3, tag=name + ", cap 3", stage=False)
    assert eng.info("memo0_active") == 1 and eng.info("memo1_active") == 1
    assert eng.info("memo0_bytes") > 0


@pytest.mark.parametrize("waves", ["8", "default"])
def test_evidence_sequence_on_one_engine_20x30(Engine, oracle_mod, grid20x30, monkeypatch, waves):
    g = grid20x30
    if waves == "8":
        monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    with Engine(g) as eng:
        _force_resident(eng)
        assert eng.info("resident_blocks") > 1 and (waves != "8" or eng.info("resident_waves") == 8)
        assert eng.info("memo1_active") == 0    # built by the first run that can use it
        _run_sequence(eng, oracle_mod, g)
        sets = dict(_evidence_sets(eng, g))
        eng.set_option("direct", 0)             # the service-block barrier reads the same image
        _check(eng, oracle_mod, g, sets["B"], 1e-6, tag="direct 0")
        eng.set_option("direct", 1)


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
            _check(eng, oracle_mod, g, ev, 1e-12, 3, tag=name + ", cap 3", stage=False)


@pytest.mark.parametrize("k", [2, 3])
def test_evidence_sequence_small_arities(Engine, oracle_mod, monkeypatch, k):
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = synth.grid(20, 30, k, seed=2030 + k)
    with Engine(g) as eng:
        _force_resident(eng)
        _run_sequence(eng, oracle_mod, g)


def test_more_than_two_children_per_node(Engine, oracle_mod):
    """A DAG with <= 2 parents and up to 8 children per node, dense layout: nodes whose rings have up to ten members and whose
    pi-messages go to more than two records."""
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
            kid = int(next(v for v in range(d.n) if busy in d.in_idx[d.in_ptr[v]:d.in_ptr[v + 1]]))   # a child of the busy node
            evs = [None, Evidence.from_dict(d, {busy: 0, leaf: k - 1}), synth.random_evidence(d, 0.03, seed=seed),
                   Evidence.from_dict(d, {busy: np.full(k, 1.0 / k), kid: 0}), None, Evidence.from_dict(d, {kid: k - 1, leaf: k - 1})]
            for i, ev in enumerate(evs):
                _check(eng, oracle_mod, d, ev, 1e-6, tag=f"seed {seed} set {i}")
                _check(eng, oracle_mod, d, ev, 1e-12, 3, tag=f"seed {seed} set {i} cap 3", stage=False)
            done += 1
            if done == 2:
                break
    assert done >= 1


def test_stop_rules(Engine, oracle_mod, grid20x30, monkeypatch):
    """The residuals of the 20 x 30 grid begin 0.9197, 0.1333, 0.07342 without evidence and differently with the 1 % set: eps just
    above each makes the oracle stop after 1, 2 and 3 sweeps, as do max_sweeps 1, 2 and 3.  A run never starts behind a sweep that
    may be its last: depth 0, at most 1, at most 2 -- and 2 only where eps is at most the policy's seed."""
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    ev1 = synth.random_evidence(g, 0.01, seed=7)
    with Engine(g) as eng:
        _force_resident(eng)
        for name, ev, eps3 in (("none", None, (1.38, 0.1999, 0.1101)), ("1 %", ev1, (1.5, 0.234, 0.1318))):
            _check(eng, oracle_mod, g, ev, 1e-6, tag=name)   # (builds the images; from sweep 2)
            for want, eps in zip((1, 2, 3), eps3):
                o = _oracle(oracle_mod, g, ev, eps, 0)
                assert o["sweeps"] == want, (name, eps, o["sweeps"], o["residuals"][:4])
                st = _check(eng, oracle_mod, g, ev, eps, depth=range(0, want), tag=f"{name} eps {eps}", stage=False)
                # sweep `want - 1` ended the run: it was executed, and its residual is below eps -- so is the seed of a stored sweep
                # that is a lower bound of the sweep's residual; the stored sweeps in front of it had residuals of at least eps
                assert st["memo_depth"] == (0 if want == 1 else st["memo_depth"])
            for cap in (1, 2, 3):
                _check(eng, oracle_mod, g, ev, 1e-12, cap, depth=max(cap - 1, 0), tag=f"{name} cap {cap}", stage=False)
            _check(eng, oracle_mod, g, ev, 1e-6, tag=name + " again", stage=False)


def test_work_limit(Engine, oracle_mod, grid20x30, monkeypatch):
    """A set over the work limit does not patch the second-sweep image: runs start at sweep 1, same bits; the sparse set behind it
    restores what the image still held from the set before the skipped one, and runs start at sweep 2 again."""
    from bayesiannetwork_amd import Evidence, synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    monkeypatch.setenv("BN_MEMO1_LIMIT", "1000")     # (200 listed nodes of the grid, five threads each)
    g = grid20x30
    k = int(g.k[0])
    sparse0 = synth.random_evidence(g, 0.02, seed=3)
    dense = Evidence.from_dict(g, {v: v % k for v in range(0, g.n, 2)})   # every second node
    sparse1 = synth.random_evidence(g, 0.02, seed=4)
    with Engine(g) as eng:
        _force_resident(eng)
        _check(eng, oracle_mod, g, sparse0, 1e-6, tag="sparse")
        _check(eng, oracle_mod, g, dense, 1e-6, depth=1, tag="dense")
        assert eng.info("memo1_active") == 0 and eng.info("memo0_active") == 1
        _check(eng, oracle_mod, g, dense, 1e-12, 3, depth=1, tag="dense cap 3", stage=False)
        _check(eng, oracle_mod, g, sparse1, 1e-6, tag="sparse behind dense")
        assert eng.info("memo1_active") == 1
        _check(eng, oracle_mod, g, sparse1, 1e-12, 3, tag="sparse behind dense, cap 3", stage=False)
        _check(eng, oracle_mod, g, None, 1e-12, 3, tag="none behind it")


def test_options(Engine, oracle_mod, grid20x30, monkeypatch):
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    evA, evB = synth.random_evidence(g, 0.02, seed=11), synth.random_evidence(g, 0.02, seed=12)
    with Engine(g) as eng:
        _force_resident(eng)
        _check(eng, oracle_mod, g, evA, 1e-6, tag="on")
        eng.set_option("memo1", 0)
        assert eng.info("memo1_active") == 0
        _check(eng, oracle_mod, g, evA, 1e-6, depth=1, tag="memo1 0", stage=False)
        _check(eng, oracle_mod, g, evB, 1e-6, depth=1, tag="memo1 0, B")
        eng.set_option("memo1", 1)
        _check(eng, oracle_mod, g, evB, 1e-12, 3, tag="memo1 1", stage=False)   # (the image was kept right while the option was off)
        eng.set_option("memo0", 0)
        _check(eng, oracle_mod, g, evA, 1e-6, depth=0, tag="memo0 0")
        eng.set_option("memo0", 1)
        _check(eng, oracle_mod, g, evA, 1e-12, 3, tag="memo0 1", stage=False)
    monkeypatch.setenv("BN_MEMO0", "0")
    with Engine(g) as eng:
        _force_resident(eng)
        _check(eng, oracle_mod, g, evA, 1e-6, depth=0, tag="BN_MEMO0=0")
        assert eng.info("memo0_active") == 0 and eng.info("memo1_active") == 0 and eng.info("memo0_bytes") == 0
    monkeypatch.delenv("BN_MEMO0")
    monkeypatch.setenv("BN_MEMO1", "0")
    with Engine(g) as eng:
        _force_resident(eng)
        _check(eng, oracle_mod, g, evA, 1e-6, depth=1, tag="BN_MEMO1=0")
        eng.set_option("memo1", 1)                                             # turned on later: both images are built again
        _check(eng, oracle_mod, g, evB, 1e-6, tag="memo1 on later")
        _check(eng, oracle_mod, g, evB, 1e-12, 3, tag="memo1 on later, cap 3", stage=False)


def test_reload_cpt_rebuilds_both_images(Engine, oracle_mod, grid20x30, monkeypatch):
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    g2 = synth.grid(20, 30, 4, seed=77)    # the same structure, other tables
    assert np.array_equal(g.in_idx, g2.in_idx) and not np.array_equal(g.cpt, g2.cpt)
    ev = synth.random_evidence(g, 0.03, seed=8)
    with Engine(g) as eng:
        _force_resident(eng)
        _check(eng, oracle_mod, g, ev, 1e-6)
        assert eng.info("memo0_active") == 1 and eng.info("memo1_active") == 1
        eng.reload_cpt(g2.cpt)
        assert eng.info("memo0_active") == 0 and eng.info("memo1_active") == 0
        _check(eng, oracle_mod, g2, ev, 1e-6, tag="new tables", stage=False)
        assert eng.info("memo0_active") == 1 and eng.info("memo1_active") == 1
        _check(eng, oracle_mod, g2, ev, 1e-12, 3, tag="new tables, cap 3", stage=False)
        _check(eng, oracle_mod, g2, None, 1e-12, 3, tag="new tables, none")


def test_other_paths_between_runs(Engine, oracle_mod, grid20x30, monkeypatch):
    """Resident path, the same evidence on the per-sweep launches, the resident path again, then a batch of two sets."""
    from bayesiannetwork_amd import Evidence, synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    ev = synth.random_evidence(g, 0.03, seed=9)
    evs = [synth.random_evidence(g, 0.05, seed=6), Evidence.from_dict(g, {0: 3, 599: 0})]
    with Engine(g) as eng:
        _force_resident(eng)
        _check(eng, oracle_mod, g, ev, 1e-6)
        o = _oracle(oracle_mod, g, ev, 1e-6, 0)
        eng.set_option("multisweep", 0)
        r = eng.bp_run_device(1e-6)
        assert eng.last_path() == 0 and eng.bp_stats()["memo_depth"] == 0
        assert r["sweeps"] == o["sweeps"] and np.array_equal(eng.bp_beliefs(), o["beliefs"]) and np.array_equal(eng.bp_residuals(), o["residuals"])
        eng.set_option("multisweep", 2)
        _check(eng, oracle_mod, g, ev, 1e-6, tag="resident again", stage=False)
        want = [_oracle(oracle_mod, g, e, 1e-6, 0) for e in evs]
        out = eng.bp_run_batch(evs, 1e-6)
        assert eng.last_path() == 2 and eng.bp_stats()["memo_depth"] == 0
        for q, w in enumerate(want):
            assert out["sweeps"][q] == w["sweeps"] and np.array_equal(out["beliefs"][q], w["beliefs"]), f"set {q}"
        _check(eng, oracle_mod, g, ev, 1e-12, 3, tag="after the batch")
        for e in evs:
            _check(eng, oracle_mod, g, e, 1e-6, tag="a set of the batch alone")


def test_run_of_two_launches(Engine, oracle_mod, grid20x30, monkeypatch):
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    ev = synth.random_evidence(g, 0.02, seed=5)
    with Engine(g) as eng:
        _force_resident(eng)
        o = _oracle(oracle_mod, g, ev, 0.0, 1030)
        assert o["sweeps"] == 1030
        _check(eng, oracle_mod, g, ev, 0.0, 1030, launches=2)
        _check(eng, oracle_mod, g, ev, 0.0, 1030, launches=2, stage=False)


def test_one_shot_calls(Engine, oracle_mod, grid20x30, monkeypatch):
    """bn_bp_run_view with a different set on each call: the set arrives with its single run, and the engine decides whether the
    ring is worth a launch -- same bits either way, and a staged set behind them starts at sweep 2 again."""
    from bayesiannetwork_amd import synth
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")
    g = grid20x30
    evs = [synth.random_evidence(g, 0.02, seed=21), None, synth.random_evidence(g, 0.03, seed=22), synth.random_evidence(g, 0.02, seed=21)]
    with Engine(g) as eng:
        _force_resident(eng)
        for cap in (0, 3):
            for i, ev in enumerate(evs):
                eps = 1e-6 if cap == 0 else 1e-12
                o = _oracle(oracle_mod, g, ev, eps, cap)
                r = eng.bp_run_view(ev, eps, cap)
                _compare(eng, r, np.array(r["beliefs"]), o, (1, 2), 1, f"view {i} cap {cap}")
        _check(eng, oracle_mod, g, evs[2], 1e-12, 3, tag="staged behind the one-shot calls")
