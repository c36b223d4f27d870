"""Max-product entry points (bn_mpe_*) without a GPU: what a BN_DEVICE_HOST_ONLY engine answers -- argument checks with the texts of the
bn_bp_* calls, the limit text of a network no form takes, the form the path choice gives, the option's range."""
import ctypes

import numpy as np
import pytest

from bayesiannetwork_amd import Evidence, from_parent_lists, synth


@pytest.fixture(scope="module")
def E(bnlib):
    from bayesiannetwork_amd import _lib, engine
    return lambda m, **kw: engine.Engine(m, device=_lib.BN_DEVICE_HOST_ONLY, **kw)


def _mpe_raw(e, ne, node, off, val, max_sweeps=5, mm=True, st=True):
    """bn_mpe_run with hand-made (possibly malformed) arrays; returns (code, bn_last_error)."""
    from bayesiannetwork_amd import _lib
    L = _lib.lib()
    i32, f64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    node = None if node is None else np.ascontiguousarray(node, np.int32)
    off = None if off is None else np.ascontiguousarray(off, np.int32)
    val = None if val is None else np.ascontiguousarray(val, np.float64)
    out_mm, out_st = np.zeros(int(e.model.k.sum())), np.zeros(e.model.n, np.int32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    rc = L.bn_mpe_run(e._h, ne, p(node, i32), p(off, i32), p(val, f64), 1e-3, max_sweeps, p(out_mm, f64) if mm else None,
                      p(out_st, i32) if st else None, None, None, None)
    return rc, L.bn_last_error().decode()


def test_no_max_product_without_gpu(E):
    from bayesiannetwork_amd import _lib
    e = E(synth.pearl())
    assert e.info("mpe_form") == 1 and e.info("mpe_last_form") == 0
    with pytest.raises(_lib.BnError, match="BN_DEVICE_HOST_ONLY") as ei:
        e.mpe_run(None, 1e-3, 5)
    assert ei.value.code == _lib.BN_ERR_STATE
    with pytest.raises(_lib.BnError) as ei:
        e.mpe_run_batch([None, Evidence.from_dict(e.model, {0: 1})], 1e-3, 5)
    assert ei.value.code == _lib.BN_ERR_STATE
    for call in (lambda: e.mpe_residuals(0), e.mpe_messages):
        with pytest.raises(_lib.BnError) as ei:
            call()
        assert ei.value.code == _lib.BN_ERR_STATE


def test_malformed_evidence_has_the_bp_texts(E):
    from bayesiannetwork_amd import _lib
    e = E(synth.pearl())   # four binary nodes
    cases = [((-1, None, None, None), "negative evidence count"),
             ((1, None, [0, 2], [1.0, 0.0]), "null evidence array"),
             ((1, [0], [1, 3], [1.0, 0.0, 0.0]), r"ev_off\[0\] != 0"),
             ((1, [4], [0, 2], [1.0, 0.0]), "evidence node out of range"),
             ((2, [1, 1], [0, 2, 4], [1.0, 0.0, 1.0, 0.0]), "evidence node listed twice"),
             ((1, [2], [0, 3], [1.0, 0.0, 0.0]), "evidence vector of node 2 must have selectable_num entries"),
             ((1, [2], [0, 2], None), "null ev_val")]
    import re
    for args, text in cases:
        rc, msg = _mpe_raw(e, *args)
        assert rc == _lib.BN_ERR_ARG and re.search(text, msg), (args, rc, msg)
    rc, msg = _mpe_raw(e, 0, None, None, None, max_sweeps=-1)
    assert rc == _lib.BN_ERR_ARG and msg == "max_sweeps < 0"
    assert _mpe_raw(e, 0, None, None, None, mm=False)[0] == _lib.BN_ERR_ARG
    assert _mpe_raw(e, 0, None, None, None, st=False)[0] == _lib.BN_ERR_ARG
    # a batch: the set count's range, the counts array
    L = _lib.lib()
    out_mm, out_st = np.zeros(8), np.zeros(4, np.int32)
    f64, i32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    for n_sets in (0, _lib.BN_MAX_BATCH_SETS + 1):
        rc = L.bn_mpe_run_batch(e._h, n_sets, None, None, None, None, 1e-3, 5, out_mm.ctypes.data_as(f64), out_st.ctypes.data_as(i32), None, None, None)
        assert rc == _lib.BN_ERR_ARG and "n_sets must be in 1.." in L.bn_last_error().decode()
    rc = L.bn_mpe_run_batch(e._h, 1, None, None, None, None, 1e-3, 5, out_mm.ctypes.data_as(f64), out_st.ctypes.data_as(i32), None, None, None)
    assert rc == _lib.BN_ERR_ARG and L.bn_last_error().decode() == "null ne"
    # well-formed evidence passes the checks and reaches the "no GPU" answer
    rc, msg = _mpe_raw(e, 1, [2], [0, 2], [1.0, 0.0])
    assert rc == _lib.BN_ERR_STATE and "BN_DEVICE_HOST_ONLY" in msg


def test_nine_parents_name_the_limit(E):
    from bayesiannetwork_amd import _lib
    m = 9
    rng = np.random.default_rng(5)
    t = 0.1 + rng.random((2 ** m, 2))
    model = from_parent_lists(k=[2] * (m + 1), parents=[[] for _ in range(m)] + [list(range(m))],
                              cpts=[[0.5, 0.5]] * m + [(t / t.sum(axis=1, keepdims=True)).ravel().tolist()], name="nine_parents")
    e = E(model)
    assert e.info("mpe_form") == 0
    with pytest.raises(_lib.BnError, match="more than 8 parents") as ei:
        e.mpe_run(None, 1e-3, 5)
    assert ei.value.code == _lib.BN_ERR_STATE


def test_form_choice_and_option(E):
    from bayesiannetwork_amd import _lib
    small = E(synth.pearl())
    assert small.info("small_eligible") == 1 and small.info("mpe_form") == 1
    mid = E(synth.random_dag(300, 3, 16, [2, 3, 4, 3, 2, 4, 5], seed=12))
    assert mid.info("small_eligible") == 0 and mid.info("mid_eligible") == 1 and mid.info("mpe_form") == 2
    mid.set_option("mpe_form", 1)            # forcing a form the network is not eligible for: none, and the run says why
    assert mid.info("mpe_form") == 0
    with pytest.raises(_lib.BnError, match="mpe_form = 1") as ei:
        mid.mpe_run(None, 1e-3, 5)
    assert ei.value.code == _lib.BN_ERR_STATE
    mid.set_option("mpe_form", 0)
    assert mid.info("mpe_form") == 2
    for bad in (-1, 3):
        with pytest.raises(_lib.BnError) as ei:
            mid.set_option("mpe_form", bad)
        assert ei.value.code == _lib.BN_ERR_ARG
    with pytest.raises(_lib.BnError):
        mid.set_option("mpe_nonsense", 1)
    sharded = E(synth.grid(12, 12, 4, seed=2), rank=0, nranks=2)
    with pytest.raises(_lib.BnError, match="sharded") as ei:
        sharded.mpe_run(None, 1e-3, 5)
    assert ei.value.code == _lib.BN_ERR_STATE
