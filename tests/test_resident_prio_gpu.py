"""Issue priority between the two waves of a SIMD in the resident kernel's grid-barrier form (bn_resident.hip prio_segment): waves w
and w + 4 of a block exchange priority at the fences of a sweep.  Priority is timing only, so everything the caller sees must be
what the oracle computes, bit for bit: sweep count, the whole residual history, beliefs and both message arrays.  The shapes are the
smallest at which the schedule could go wrong: a block whose partners are not both at work (one of a pair idles through the barriers),
a full block beside a one-tile block, the four-waves-per-block instantiation (no partner: no priority code), a one-block grid (LDS-only
barrier), and the other lean instantiations (one parent, k = 2, k = 3), which carry the same fences.  Each shape runs without evidence
and with a sparse set, cut off behind sweep 1 and 2 and to convergence, once behind the stored sweeps (a launch then begins at sweep
0, 1 or 2 by the cap) and once with both images off (every launch begins at sweep 0).  Helpers as tests/test_resident_memo1_gpu.py."""
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


_ORACLE = {}


def _oracle(oracle_mod, g, ev, eps, max_sweeps):
    """One oracle run per (network, set, eps, cap), shared by the two passes over the images."""
    key = (g.name, None if ev is None else (ev.node.tobytes(), ev.val.tobytes()), eps, max_sweeps)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_mod.bp_run(g, ev, eps, max_sweeps, dump_msgs=True)
    return _ORACLE[key]


def _force_resident(eng):
    eng.set_option("small", 0)
    eng.set_option("mid", 0)
    eng.set_option("multisweep", 2)
    eng.set_option("flow", 0)      # the grid barrier: every wave leaves it at the same moment
    eng.set_option("direct", 1)
    assert eng.info("resident_eligible") == 1


def _check(eng, oracle_mod, g, ev, eps, max_sweeps, launches, tag):
    o = _oracle(oracle_mod, g, ev, eps, max_sweeps)
    eng.bp_set_evidence(ev)
    r = eng.bp_run_device(eps, max_sweeps)
    st = eng.bp_stats()
    assert eng.last_path() == 2 and eng.info("last_flow") == 0, tag
    assert st["resident_aborts"] == 0, tag
    assert st["sweep_launches"] == launches, (tag, st["sweep_launches"])
    assert r["sweeps"] == o["sweeps"], (tag, r["sweeps"], o["sweeps"])
    assert np.array_equal(eng.bp_residuals(), o["residuals"]), (tag, eng.bp_residuals()[:4], o["residuals"][:4])
    assert np.array_equal(eng.bp_beliefs(), o["beliefs"], equal_nan=True), tag
    pi, lam = eng.bp_messages()
    assert np.array_equal(pi, o["pi_msg"], equal_nan=True) and np.array_equal(lam, o["lambda_msg"], equal_nan=True), tag
    return st


# name -> (network, BN_RESIDENT_WAVES, waves per block expected, tiles expected).  A tile holds nodes of one parent count: the root,
# the first row and column, then the two-parent nodes
def _shapes():
    from bayesiannetwork_amd import synth
    return {
        "grid20x30_k4": (lambda: synth.grid(20, 30, 4, seed=2030), "8", 8, 11),     # the second block has tiles in waves 0-2 only
        "grid23x23_k4_w8": (lambda: synth.grid(23, 23, 4, seed=2323), "8", 8, 10),  # a full block and a two-tile block
        "grid22x22_k4_w8": (lambda: synth.grid(22, 22, 4, seed=2222), "8", 8, 9),   # a full block and a one-tile block
        "grid23x23_k4_w4": (lambda: synth.grid(23, 23, 4, seed=2323), "4", 4, 10),  # the whole-register-file instantiation
        "grid8x8_k4": (lambda: synth.grid(8, 8, 4, seed=88), "8", 8, 3),            # one block: LDS-only barrier
        "chain200_k4": (lambda: synth.grid(1, 200, 4, seed=200), "8", 8, 5),        # one parent
        "grid20x30_k2": (lambda: synth.grid(20, 30, 2, seed=2032), "8", 8, 11),
        "grid20x30_k3": (lambda: synth.grid(20, 30, 3, seed=2033), "8", 8, 11),
    }


_SHAPES = ["grid20x30_k4", "grid23x23_k4_w8", "grid22x22_k4_w8", "grid23x23_k4_w4", "grid8x8_k4", "chain200_k4", "grid20x30_k2", "grid20x30_k3"]
_NETS = {}


def _net(shape):
    make, waves, per_block, tiles = _shapes()[shape]
    if shape not in _NETS:
        _NETS[shape] = make()
    return _NETS[shape], waves, per_block, tiles


@pytest.mark.parametrize("images", ["default", "off"])
@pytest.mark.parametrize("shape", _SHAPES)
def test_bit_identical_to_the_oracle(Engine, oracle_mod, monkeypatch, shape, images):
    from bayesiannetwork_amd import synth
    g, waves, per_block, tiles = _net(shape)
    monkeypatch.setenv("BN_RESIDENT_WAVES", waves)
    if images == "off":
        monkeypatch.setenv("BN_MEMO0", "0")
        monkeypatch.setenv("BN_MEMO1", "0")
    sparse = synth.random_evidence(g, 0.03, seed=7)
    assert sparse.node.shape[0] >= 1
    with Engine(g) as eng:
        _force_resident(eng)
        assert eng.info("resident_waves") == per_block, eng.info("resident_waves")
        assert int(np.asarray(eng.node_tiles()).max()) + 1 == tiles
        assert (eng.info("resident_blocks") == 1) == (tiles <= per_block), eng.info("resident_blocks")
        depths = set()
        for name, ev in (("none", None), ("sparse", sparse)):
            # to convergence first (the run that builds the images), then cut off behind sweep 1 and 2, then to convergence again: behind
            # the images these launches begin at sweep 0, 1 and 2
            for cap in (0, 1, 2, 0):
                st = _check(eng, oracle_mod, g, ev, 1e-6, cap, 1, f"{shape} {images} {name} cap {cap}")
                depths.add(st["memo_depth"])
            if shape == "grid20x30_k4":   # a run of two launches: the second begins in the middle of the run
                o = _oracle(oracle_mod, g, ev, 0.0, 1030)
                assert o["sweeps"] == 1030
                _check(eng, oracle_mod, g, ev, 0.0, 1030, 2, f"{shape} {images} {name} eps 0 cap 1030")
        if images == "off":
            assert depths == {0}, (shape, depths)
        elif shape == "grid20x30_k4":     # (the depths on this grid are pinned by tests/test_resident_memo1_gpu.py)
            assert depths == {0, 1, 2}, (shape, depths)
