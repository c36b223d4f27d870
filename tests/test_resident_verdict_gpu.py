"""The verdict of the resident kernel's grid barrier, direct collection (bn_resident.hip wait_verdict): the collecting wave of every tile
block decides by a vote over its lanes' partial maxima instead of reducing them first, and the residual's VALUE -- the history and the
final residual -- is recorded off the tiles' path: by a wave without a tile of the last tile-carrying block where there is one (tiles
no multiple of the waves per block), else by block 0's collecting wave behind its verdict.  Nothing the caller sees may change: sweep
count, the whole residual history, the final residual, beliefs and both message arrays are the oracle's, bit for bit.

Shapes, the smallest that reach each branch (tiles of an r x c grid: 1 + ceil((r + c - 2) / 64) + ceil((r - 1)(c - 1) / 64)):
  22 x 22,  9 tiles: eight waves per block -- a full block and a block with one tile; four -- the third block has one tile: a recorder
  30 x 30, 16 tiles: two full blocks of eight, four of four: no wave without a tile beside a tile, block 0 records
  128 x 128, 258 tiles at four waves per block: more than 64 blocks, a lane collects more than one block's granules (four-load sweep)
  20 x 30, 11 tiles: the run of two launches the project's other resident tests use (1 030 sweeps)
Helpers as tests/test_resident_prio_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _resident_tiles(monkeypatch):
    monkeypatch.setenv("BN_DAG", "0")   # k = 4 networks would take the register-resident DAG path by default
    for name in ("BN_MEMO0", "BN_MEMO1", "BN_MEMO1_LIMIT", "BN_MEMO1_ONESHOT", "BN_RESIDENT_WAVES", "BN_RESIDENT_DIRECT"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def Engine(bnlib):
    from bayesiannetwork_amd.engine import Engine
    return Engine


_ORACLE = {}


def _oracle(oracle_mod, g, ev, eps, max_sweeps):
    """One oracle run per (network, set, eps, cap), shared by the cases that repeat it."""
    key = (g.name, None if ev is None else (ev.node.tobytes(), ev.val.tobytes()), eps, max_sweeps)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.bp_run(g, ev, eps, max_sweeps, dump_msgs=True)
    return _ORACLE[key]


def _force_resident(eng, direct=1):
    eng.set_option("small", 0)
    eng.set_option("mid", 0)
    eng.set_option("multisweep", 2)
    eng.set_option("flow", 0)      # the grid barrier
    eng.set_option("direct", direct)
    assert eng.info("resident_eligible") == 1


def _check(eng, oracle_mod, g, ev, eps, max_sweeps=0, launches=1, tag="", stage=True, depth=None):
    o = _oracle(oracle_mod, g, ev, eps, max_sweeps)
    if stage:
        eng.bp_set_evidence(ev)
    r = eng.bp_run_device(eps, max_sweeps)
    st = eng.bp_stats()
    assert eng.last_path() == 2 and eng.info("last_flow") == 0, tag
    assert st["resident_aborts"] == 0, tag
    assert st["sweep_launches"] == launches, (tag, st["sweep_launches"])
    if depth is not None:
        assert st["memo_depth"] == depth, (tag, st["memo_depth"])
    assert r["sweeps"] == o["sweeps"], (tag, r["sweeps"], o["sweeps"])
    hist = eng.bp_residuals()
    assert hist.shape == o["residuals"].shape and np.array_equal(hist, o["residuals"]), (tag, hist[:4], o["residuals"][:4])
    assert r["residual"] == o["residuals"][-1], (tag, r["residual"], o["residuals"][-1])
    assert np.array_equal(eng.bp_beliefs(), o["beliefs"], equal_nan=True), tag
    pi, lam = eng.bp_messages()
    assert np.array_equal(pi, o["pi_msg"], equal_nan=True) and np.array_equal(lam, o["lambda_msg"], equal_nan=True), tag
    return o


# name -> (rows, columns, seed, BN_RESIDENT_WAVES, tiles, tile blocks of the launch: rounded up to a multiple of eight, whether a wave
# without a tile stands beside a tile in the last tile-carrying block: the recorder)
_SHAPES = {
    "grid22x22_w8": (22, 22, 2222, "8", 9, 8, True),
    "grid22x22_w4": (22, 22, 2222, "4", 9, 8, True),
    "grid30x30_w8": (30, 30, 3030, "8", 16, 8, False),
    "grid30x30_w4": (30, 30, 3030, "4", 16, 8, False),
    "grid128x128_w4": (128, 128, 128128, "4", 258, 72, True),
    "grid20x30_w8": (20, 30, 2030, "8", 11, 8, True),
}
_SMALL = ["grid22x22_w8", "grid22x22_w4", "grid30x30_w8", "grid30x30_w4"]
_NETS = {}


def _net(shape):
    from bayesiannetwork_amd import synth
    rows, cols, seed = _SHAPES[shape][:3]
    if (rows, cols) not in _NETS:
        _NETS[(rows, cols)] = synth.grid(rows, cols, 4, seed=seed)
    return _NETS[(rows, cols)]


def _engine(Engine, monkeypatch, shape, direct=1):
    """An engine forced onto the form under test, its launch shape (waves per block, tiles, blocks) pinned.  Which of the two
    recording branches the kernel takes follows from that shape by has_recorder's rule and is not observable from the host: both
    give the same bits, and the last column only records which one the rule selects."""
    _, _, _, waves, tiles, blocks, recorder = _SHAPES[shape]
    monkeypatch.setenv("BN_RESIDENT_WAVES", waves)
    eng = Engine(_net(shape))
    _force_resident(eng, direct)
    assert eng.info("resident_waves") == int(waves), eng.info("resident_waves")
    assert int(np.asarray(eng.node_tiles()).max()) + 1 == tiles
    assert eng.info("resident_blocks") == blocks, eng.info("resident_blocks")
    assert (tiles % int(waves) != 0) == recorder
    return eng


def _sparse(g):
    from bayesiannetwork_amd import synth
    ev = synth.random_evidence(g, 0.03, seed=7)
    assert ev.node.shape[0] >= 1
    return ev


@pytest.mark.parametrize("shape", _SMALL + ["grid128x128_w4"])
def test_bit_identical_to_the_oracle(Engine, oracle_mod, monkeypatch, shape):
    g = _net(shape)
    with _engine(Engine, monkeypatch, shape) as eng:
        for name, ev in (("none", None), ("sparse", _sparse(g))):
            _check(eng, oracle_mod, g, ev, 1e-6, tag=f"{shape} {name}")
            _check(eng, oracle_mod, g, ev, 1e-6, 3, tag=f"{shape} {name} cap 3", stage=False)


def _edges(o):
    """Two sweeps j >= 1 of a history whose residual is below every earlier one: eps just above h[j] stops the run on sweep j."""
    h = o["residuals"]
    js = [j for j in range(1, len(h) - 1) if h[j] < h[:j].min()]
    assert len(js) >= 2, h[:8]
    return h, (js[0], js[len(js) // 2] if js[len(js) // 2] != js[0] else js[-1])


def _stop_rules(eng, oracle_mod, g, ev, tag):
    o = _check(eng, oracle_mod, g, ev, 1e-6, tag=tag)
    h, (j0, j1) = _edges(o)
    assert j0 != j1
    for j in (j0, j1):
        # the strict '<': a residual EQUAL to eps does not stop the run, the next double above it does
        at = _check(eng, oracle_mod, g, ev, float(h[j]), tag=f"{tag} eps = h[{j}]", stage=False)
        assert at["sweeps"] > j + 1, (tag, j, at["sweeps"])
        above = _check(eng, oracle_mod, g, ev, float(np.nextafter(h[j], np.inf)), tag=f"{tag} eps = next(h[{j}])", stage=False)
        assert above["sweeps"] == j + 1, (tag, j, above["sweeps"])
    for cap in (1, 2, 3, o["sweeps"] + 5):
        c = _check(eng, oracle_mod, g, ev, 1e-6, cap, tag=f"{tag} cap {cap}", stage=False)
        assert c["sweeps"] == min(cap, o["sweeps"]), (tag, cap, c["sweeps"])
    z = _check(eng, oracle_mod, g, ev, 0.0, 12, tag=f"{tag} eps 0 cap 12", stage=False)   # eps = 0 never converges: the cap ends it
    assert z["sweeps"] == 12, (tag, z["sweeps"])


@pytest.mark.parametrize("shape", _SMALL)
def test_stop_rules(Engine, oracle_mod, monkeypatch, shape):
    g = _net(shape)
    with _engine(Engine, monkeypatch, shape) as eng:
        _stop_rules(eng, oracle_mod, g, _sparse(g), shape)


def _memo_depths(eng, oracle_mod, g, ev, tag):
    """Runs that begin at sweep 2, 1 and 0 (behind the second-sweep image, the first-sweep image, no image): the history the launch
    reports begins that many entries into the run's."""
    _check(eng, oracle_mod, g, ev, 1e-6, tag=f"{tag} depth 2", depth=2)
    _check(eng, oracle_mod, g, ev, 1e-12, 3, tag=f"{tag} depth 2, cap 3", stage=False, depth=2)
    eng.set_option("memo1", 0)
    _check(eng, oracle_mod, g, ev, 1e-6, tag=f"{tag} depth 1", stage=False, depth=1)
    _check(eng, oracle_mod, g, ev, 1e-12, 2, tag=f"{tag} depth 1, cap 2", stage=False, depth=1)
    eng.set_option("memo0", 0)
    _check(eng, oracle_mod, g, ev, 1e-6, tag=f"{tag} depth 0", depth=0)
    _check(eng, oracle_mod, g, ev, 1e-12, 1, tag=f"{tag} depth 0, cap 1", stage=False, depth=0)


@pytest.mark.parametrize("shape", _SMALL)
def test_each_memo_depth(Engine, oracle_mod, monkeypatch, shape):
    g = _net(shape)
    with _engine(Engine, monkeypatch, shape) as eng:
        _memo_depths(eng, oracle_mod, g, _sparse(g), shape)


def _other_evidence(eng, oracle_mod, g, tag):
    from bayesiannetwork_amd import synth
    for name, ev in (("A", synth.random_evidence(g, 0.02, seed=11)), ("B", synth.random_evidence(g, 0.02, seed=12)), ("none", None)):
        _check(eng, oracle_mod, g, ev, 1e-6, tag=f"{tag} set {name}")
        _check(eng, oracle_mod, g, ev, 1e-9, tag=f"{tag} set {name} again, eps 1e-9", stage=False)


@pytest.mark.parametrize("shape", _SMALL)
def test_second_run_with_other_evidence(Engine, oracle_mod, monkeypatch, shape):
    """Generations count on from run to run on one engine: a granule left by an earlier run never carries a wanted generation."""
    with _engine(Engine, monkeypatch, shape) as eng:
        _other_evidence(eng, oracle_mod, _net(shape), shape)


def _two_launches(eng, oracle_mod, g):
    for name, ev in (("none", None), ("sparse", _sparse(g))):
        o = _oracle(oracle_mod, g, ev, 0.0, 1030)
        assert o["sweeps"] == 1030
        _check(eng, oracle_mod, g, ev, 0.0, 1030, launches=2, tag=f"20x30 {name} eps 0 cap 1030")
        _check(eng, oracle_mod, g, ev, 1e-6, tag=f"20x30 {name} behind it", stage=False)


def test_run_beyond_one_launch(Engine, oracle_mod, monkeypatch):
    """1 030 sweeps are two launches (a launch executes at most 1 024): the second launch's history continues the first's."""
    with _engine(Engine, monkeypatch, "grid20x30_w8") as eng:
        _two_launches(eng, oracle_mod, _net("grid20x30_w8"))


@pytest.mark.parametrize("shape", ["grid22x22_w8", "grid30x30_w8"])
def test_service_block_collector_unchanged(Engine, oracle_mod, monkeypatch, shape):
    """The same cases with `direct` 0: a service block collects the granules, records the residual and publishes the verdict."""
    g = _net(shape)
    with _engine(Engine, monkeypatch, shape, direct=0) as eng:
        _stop_rules(eng, oracle_mod, g, _sparse(g), shape + " direct 0")
        _other_evidence(eng, oracle_mod, g, shape + " direct 0")
    with _engine(Engine, monkeypatch, shape, direct=0) as eng:
        _memo_depths(eng, oracle_mod, g, _sparse(g), shape + " direct 0")
    if shape == "grid22x22_w8":
        with _engine(Engine, monkeypatch, "grid20x30_w8", direct=0) as eng:
            _two_launches(eng, oracle_mod, _net("grid20x30_w8"))
