"""Start and end of a resident launch (bn_resident.hip): the prologue that makes a tile resident (CPT image in registers and LDS,
references, evidence marks, node vectors), the launch's first sweep, which reads no messages, and finalize, which writes the beliefs
of even arities as 16-byte stores.  Everything here is compared with the oracle bit for bit: sweep count, residual history, final
messages, beliefs.  The shapes are the smallest on which a change to the start-up (such as running the first sweep while the CPT
image is still arriving) can go wrong: a 20 x 30 grid (600 nodes: full tiles and a partly filled one, more than one block, root /
one-parent / two-parent tiles), an 8 x 8 grid (one block: the LDS-only barrier), k = 2 and 3 (no CPT in LDS; 16-byte and scalar
belief stores), a run continued in a second launch (its prologue starts with sweep_begin > 0: node vectors and messages come from
memory), a batch and the dataflow form.  Every engine runs the headline instantiation: eight waves per block.
NOT YET RUN ON A GPU when it was written (EXPERIMENTS.md R11.1): the oracle side of every case was run, the device side was not."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (flow, direct): the grid barrier collected by every tile block (what the headline runs), the dataflow form, the service block
FORMS = ((0, 1), (1, 1), (0, 0))


@pytest.fixture(autouse=True)
def _resident_tiles_at_eight_waves(monkeypatch):
    monkeypatch.setenv("BN_DAG", "0")              # k = 4 networks would take the register-resident DAG path by default
    monkeypatch.setenv("BN_RESIDENT_WAVES", "8")   # ... and networks this small four waves per block (CPT entirely in registers)


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
    assert eng.info("resident_eligible") == 1 and eng.info("resident_waves") == 8


def _check_against_oracle(eng, oracle_mod, g, ev, eps, max_sweeps=0, forms=FORMS, reps=2, launches=1):
    o = oracle_mod.bp_run(g, ev, eps, max_sweeps, dump_msgs=True)
    _force_resident(eng)
    for flow, direct in forms:
        eng.set_option("flow", flow)
        eng.set_option("direct", direct)
        for i in range(reps):   # the second run starts from what the first left in the buffers
            r = eng.bp_run(ev, eps, max_sweeps)
            tag = f"flow {flow} direct {direct} run {i}"
            assert eng.last_path() == 2 and eng.bp_stats()["sweep_launches"] == launches, tag
            assert eng.info("last_flow") == (flow if eng.info("flow_eligible") else 0), tag
            assert r["sweeps"] == o["sweeps"], tag
            assert np.array_equal(eng.bp_residuals(), o["residuals"]), tag
            assert np.array_equal(r["beliefs"], o["beliefs"], equal_nan=True), tag
            pi, lam = eng.bp_messages()
            assert np.array_equal(pi, o["pi_msg"], equal_nan=True) and np.array_equal(lam, o["lambda_msg"], equal_nan=True), tag
        assert eng.bp_stats()["resident_aborts"] == 0
    eng.set_option("flow", 1)
    eng.set_option("direct", 1)
    return o


def _node_of_partial_tile(eng):
    """A node (not the root) of a tile with fewer than 64 nodes."""
    tiles = eng.node_tiles()
    count = np.bincount(tiles)
    partial = [t for t in range(count.shape[0]) if 0 < count[t] < 64 and t != tiles[0]]
    assert partial, "the grid should have a partly filled tile"
    return int(np.flatnonzero(tiles == partial[-1])[-1])


def test_layout_is_the_one_these_cases_are_about(Engine, grid20x30):
    with Engine(grid20x30) as eng:
        _force_resident(eng)
        assert eng.info("resident_blocks") > 1
        assert {c["m"] for c in eng.layout_classes()} == {0, 1, 2}
        assert all(c["kv"] == 4 and c["lanes_per_node"] == 1 for c in eng.layout_classes())
        count = np.bincount(eng.node_tiles())
        assert (count == 64).any() and ((count > 0) & (count < 64)).any() and eng.layout()["n_tiles"] > 8


@pytest.mark.parametrize("case", ["none", "root", "partial_tile", "soft", "cap1", "cap2"])
def test_start_of_a_run_20x30(Engine, oracle_mod, grid20x30, case):
    from bayesiannetwork_amd import Evidence
    g = grid20x30
    with Engine(g) as eng:
        eps, cap, ev = 1e-6, 0, None
        if case == "root":
            ev = Evidence.from_dict(g, {0: 2})
        elif case == "partial_tile":
            ev = Evidence.from_dict(g, {_node_of_partial_tile(eng): 1})
        elif case == "soft":
            ev = Evidence.from_dict(g, {0: np.array([0.1, 0.2, 0.3, 0.4]), 317: np.array([0.25, 0.5, 0.0, 0.25]),
                                        _node_of_partial_tile(eng): np.array([0.7, 0.1, 0.1, 0.1])})
        elif case in ("cap1", "cap2"):   # finalize follows the first sweep directly / after one ordinary sweep
            from bayesiannetwork_amd import synth
            ev, eps, cap = synth.random_evidence(g, 0.03, seed=4), 1e-12, 1 if case == "cap1" else 2
        o = _check_against_oracle(eng, oracle_mod, g, ev, eps, cap)
        if cap:
            assert o["sweeps"] == cap
        else:
            assert o["sweeps"] > 2


def test_start_of_a_run_one_block(Engine, oracle_mod):
    from bayesiannetwork_amd import synth
    g = synth.grid(8, 8, 4, seed=88)
    ev = synth.random_evidence(g, 0.05, seed=1)
    with Engine(g) as eng:
        _force_resident(eng)
        assert eng.info("resident_blocks") == 1
        _check_against_oracle(eng, oracle_mod, g, ev, 1e-6)
        _check_against_oracle(eng, oracle_mod, g, ev, 1e-12, max_sweeps=1)


@pytest.mark.parametrize("k", [2, 3])
def test_start_of_a_run_small_arities(Engine, oracle_mod, k):
    from bayesiannetwork_amd import Evidence, synth
    g = synth.grid(20, 30, k, seed=2030 + k)
    with Engine(g) as eng:
        _check_against_oracle(eng, oracle_mod, g, synth.random_evidence(g, 0.02, seed=3), 1e-6)
        _check_against_oracle(eng, oracle_mod, g, Evidence.from_dict(g, {0: 1}), 1e-12, max_sweeps=1)


def test_second_launch_of_a_run_starts_from_memory(Engine, oracle_mod, grid20x30):
    """A launch executes at most 1024 iterations: sweep 1024 is the first of a second launch, whose prologue must load node
    vectors and read messages as any later sweep does -- nothing of the first sweep's short cuts applies."""
    from bayesiannetwork_amd import synth
    g = grid20x30
    ev = synth.random_evidence(g, 0.02, seed=5)
    with Engine(g) as eng:
        o = _check_against_oracle(eng, oracle_mod, g, ev, 0.0, max_sweeps=1030, forms=((0, 1), (1, 1)), launches=2)
        assert o["sweeps"] == 1030


def test_batch_of_two_and_flow_equal_their_single_runs(Engine, oracle_mod, grid20x30):
    from bayesiannetwork_amd import Evidence, synth
    g = grid20x30
    evs = [synth.random_evidence(g, 0.05, seed=6), Evidence.from_dict(g, {0: 3, 599: 0})]
    want = [oracle_mod.bp_run(g, ev, 1e-6) for ev in evs]
    with Engine(g) as eng:
        _force_resident(eng)
        for direct in (1, 0):
            eng.set_option("direct", direct)
            for _ in range(2):
                out = eng.bp_run_batch(evs, 1e-6)
                assert eng.last_path() == 2
                for q, o in enumerate(want):
                    assert out["sweeps"][q] == o["sweeps"], f"set {q}"
                    assert np.array_equal(out["beliefs"][q], o["beliefs"]), f"set {q}"
                    assert np.array_equal(eng.bp_residuals_batch(q), o["residuals"]), f"set {q}"
        eng.set_option("direct", 1)
        eng.set_option("flow", 1)
        for ev, o in zip(evs, want):
            r = eng.bp_run(ev, 1e-6)
            assert eng.last_path() == 2 and eng.info("last_flow") == 1
            assert r["sweeps"] == o["sweeps"] and np.array_equal(r["beliefs"], o["beliefs"])
            assert np.array_equal(eng.bp_residuals(), o["residuals"])
