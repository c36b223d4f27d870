"""CPU checks of tests/loglik_refs.py, the restatement the GPU scores are held to (tests/test_loglik_gpu.py): rows and
node sums against enumeration in exact rationals on tiny networks, `parameters` against hand-computed cases, the two
restatements against each other and against the reference's literal loop; and the host side of the library that needs no
device: the log table and `parameters` of a BN_DEVICE_HOST_ONLY engine."""
import itertools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import exact_refs
import loglik_refs as R
from bayesiannetwork_amd import _lib, from_parent_lists, synth
from bayesiannetwork_amd.dsc import load_dsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_networks():
    rng = np.random.default_rng(5)
    yield synth.pearl()
    yield synth.resume_chain()
    yield exact_refs._model([2, 3, 1, 2, 5], [[], [0], [0, 1], [1, 2], [0, 3]], rng, name="mixed5")
    yield exact_refs._model([3, 2, 2], [[], [0], [0, 1]], rng, zero_frac=0.4, name="zeros3")


def all_patterns(model):
    return np.array(list(itertools.product(*[range(int(k)) for k in model.k])), dtype=np.uint8)


def exact_row(model, pat, nodes):
    """sum over nodes of log theta: the float terms math.log gives, added exactly (Fraction) and rounded once"""
    total = Fraction(0)
    for v in nodes:
        row = 0
        for u in model.parents(v):
            row = row * int(model.k[u]) + int(pat[u])
        theta = float(model.cpt[int(model.cpt_off[v]) + row * int(model.k[v]) + int(pat[v])])
        if theta == 0.0:
            return -math.inf
        total += Fraction(math.log(theta))
    return float(total)


@pytest.mark.parametrize("model", list(tiny_networks()), ids=lambda m: m.name)
def test_rows_restatement_against_exact_enumeration(model):
    pats = all_patterns(model)
    for nodes in (None, [0], list(range(0, model.n, 2)), list(range(model.n))[::-1]):
        got = R.rows_ref(model, pats, nodes)
        sel = range(model.n) if nodes is None else nodes
        for p, pat in enumerate(pats):
            want = exact_row(model, pat, sel)
            if want == -math.inf:
                assert got[p] == -math.inf
                continue
            mags = [abs(math.log(float(model.cpt[q]))) for q in R.entry_index(model, pat[None, :])[0][list(sel)]]
            assert abs(got[p] - want) <= R.gamma(len(mags)) * math.fsum(mags)
    assert not np.isnan(R.rows_ref(model, pats)).any()
    # the order of the list does not matter, bit for bit
    assert np.array_equal(R.rows_ref(model, pats, [0, model.n - 1]), R.rows_ref(model, pats, [model.n - 1, 0]))


@pytest.mark.parametrize("model", list(tiny_networks()), ids=lambda m: m.name)
def test_nodes_restatement_against_exact_enumeration(model):
    rng = np.random.default_rng(model.n)
    pats = all_patterns(model)
    keep = [p for p in range(len(pats)) if R.rows_ref(model, pats[p:p + 1])[0] > -math.inf]   # only patterns the network can produce
    pats = pats[keep]
    counts = rng.choice(np.array([1, 3, 127, 1 << 31, 1 << 40], dtype=np.uint64), len(pats))
    L = R.log_table(model)
    N = R.family_counts_ref(model, pats, counts)
    # counts: exact integers, against a Python-int dict
    want_N = [0] * len(N)
    for pat, c in zip(pats, counts.tolist()):
        for q in R.entry_index(model, pat[None, :])[0]:
            want_N[q] += c
    assert N.tolist() == want_N
    got = R.nodes_ref(model, N, L)
    assert not np.isnan(got).any()
    for v in range(model.n):
        o0, o1 = int(model.cpt_off[v]), int(model.cpt_off[v + 1])
        exact = sum((Fraction(want_N[q]) * Fraction(float(L[q])) for q in range(o0, o1) if want_N[q]), Fraction(0))
        mags = [abs(float(want_N[q]) * float(L[q])) for q in range(o0, o1) if want_N[q]]
        bound = R.gamma(len(mags) + 1) * math.fsum(mags)
        assert abs(Fraction(float(got[v])) - exact) <= Fraction(bound) + Fraction(2.0 ** -52) * abs(exact), v
        assert abs(got[v] - R.exact_total(R.node_terms(model, N, L, v))) <= bound


def test_unseen_zero_entries_add_nothing():
    model = from_parent_lists([2, 2], [[], [0]], [[0.5, 0.5], [1.0, 0.0, 0.25, 0.75]])
    pats = np.array([[0, 0], [1, 1]], dtype=np.uint8)
    N = R.family_counts_ref(model, pats, [3, 5])
    ll = R.nodes_ref(model, N)
    assert ll[1] == 3 * math.log(1.0) + 5 * math.log(0.75) and not np.isnan(ll).any()
    N = R.family_counts_ref(model, np.array([[0, 1]], dtype=np.uint8), [1])   # a pattern the network gives probability 0
    assert R.nodes_ref(model, N)[1] == -math.inf and R.rows_ref(model, [[0, 1]])[0] == -math.inf


def test_parameters_by_hand():
    assert R.parameters_ref(synth.pearl()) == 1 + 1 + 2 + 4            # two roots, a node with one parent, one with two (all binary)
    m = from_parent_lists([3, 1, 5], [[], [0], [0, 1]], [np.full(3, 1 / 3), np.ones(3), np.full(15, 0.2)])
    assert R.parameters_ref(m) == 2 + 0 * 3 + 4 * 3 * 1
    from bayesiannetwork_amd import parameters
    assert parameters(m) == 14 and parameters(synth.pearl()) == 8
    alarm, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    by_hand = 0
    for v in range(alarm.n):
        rows = 1
        for u in alarm.parents(v):
            rows *= int(alarm.k[u])
        by_hand += (int(alarm.k[v]) - 1) * rows
    assert R.parameters_ref(alarm) == by_hand == int((alarm.cpt_off[-1] - np.sum(np.diff(alarm.cpt_off) // alarm.k)))


@pytest.mark.parametrize("model", list(tiny_networks()), ids=lambda m: m.name)
def test_the_two_restatements_and_the_reference_loop_agree(model):
    rng = np.random.default_rng(11)
    pats = all_patterns(model)
    pats = pats[[p for p in range(len(pats)) if R.rows_ref(model, pats[p:p + 1])[0] > -math.inf]]
    counts = rng.integers(1, 1000, len(pats)).astype(np.uint64)
    L = R.log_table(model)
    N = R.family_counts_ref(model, pats, counts)
    by_rows = math.fsum(float(c) * x for c, x in zip(counts.tolist(), R.rows_ref(model, pats, L=L).tolist()))
    by_nodes = math.fsum(R.nodes_ref(model, N, L).tolist())
    rows_mag = math.fsum(float(c) * abs(x) for c, x in zip(counts.tolist(), R.rows_ref(model, pats, L=L).tolist()))
    bound = R.likelihood_bound(model, N, L) + R.gamma(model.n + 2) * rows_mag
    assert abs(by_rows - by_nodes) <= bound
    table = R.table_dict(pats, counts)
    assert abs(R.reference_likelihood(model, table) + by_nodes) <= 2 * R.likelihood_bound(model, N, L)
    sub = [model.n - 1, 0]
    assert R.reference_aic(model, table, sub) == R.reference_likelihood(model, table, sub) + R.parameters_ref(model)
    size = int(counts.sum())
    assert R.reference_mdl(model, table) == R.reference_likelihood(model, table) + R.parameters_ref(model) * (math.log2(size) / 2)
    with pytest.raises(RuntimeError):
        R.reference_mdl(model, {})


# ---- the library's host side (no device) -------------------------------------------------------

def test_log_table_and_parameters_of_a_host_only_engine(bnlib):
    """bn_score_log_cpt has the bits of math.log per entry (-inf exactly at the zeros), before and after bn_reload_cpt;
    bn_get_info "parameters" is calc_parameters; scoring itself needs a device."""
    from bayesiannetwork_amd import log_cpt, parameters
    from bayesiannetwork_amd.engine import Engine
    rng = np.random.default_rng(3)
    alarm, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    for model in (alarm, exact_refs.polytree(60, arities=(2, 3, 5), zero_frac=0.3, seed=4), synth.random_dag(300, 4, 32, [2, 3, 5, 4], seed=8)):
        with Engine(model, device=_lib.BN_DEVICE_HOST_ONLY) as eng:
            L = log_cpt(eng)
            want = R.log_table(model)
            assert np.array_equal(L.view(np.uint64), want.view(np.uint64))
            assert np.array_equal(np.isneginf(L), model.cpt == 0.0) and not np.isnan(L).any()
            assert parameters(eng) == R.parameters_ref(model)
            cpt = model.cpt.copy()
            for v in range(model.n):   # new rows of the same shape
                t = exact_refs._random_table(rng, int(model.cpt_off[v + 1] - model.cpt_off[v]) // int(model.k[v]), int(model.k[v]), 0.2)
                cpt[model.cpt_off[v]:model.cpt_off[v + 1]] = t.reshape(-1)
            eng.reload_cpt(cpt)
            L2 = log_cpt(eng)
            assert np.array_equal(L2.view(np.uint64), R.log_table(eng.model).view(np.uint64)) and not np.array_equal(L, L2)


def test_scoring_a_host_only_engine_is_refused(bnlib):
    from bayesiannetwork_amd.engine import Engine
    import ctypes
    model = synth.pearl()
    out = np.zeros(model.n)
    with Engine(model, device=_lib.BN_DEVICE_HOST_ONLY) as eng:
        assert bnlib.bn_score_nodes(eng._h, None, out.ctypes.data_as(_lib.f64p), None) == _lib.BN_ERR_ARG   # null table
        assert bnlib.bn_score_log_cpt(eng._h, None) == _lib.BN_ERR_ARG
        assert b"null" in bnlib.bn_last_error()
        fake = ctypes.c_void_p(0)
        assert bnlib.bn_score_rows(eng._h, fake, 0, None, out.ctypes.data_as(_lib.f64p)) == _lib.BN_ERR_ARG


def test_scoring_kernels_do_not_spill(tmp_path):
    """Code-object metadata (scripts/kernel_resources.py) of bn_score_kernels.hip and bn_fit_kernels.hip compiled for gfx950
    with the Makefile's flags: every instantiation of the row kernel, the segment reduction and the node-sum kernel is there,
    without spills or scratch; the counting kernel the node pass shares with the CPT fit keeps its counters in 32 KiB of LDS."""
    import importlib.util
    import subprocess
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    csrc = os.path.join(ROOT, "bayesiannetwork_amd", "csrc")
    res = {}
    for src in ("bn_score_kernels", "bn_fit_kernels"):
        obj = str(tmp_path / (src + ".o"))
        p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                            "-c", os.path.join(csrc, src + ".hip"), "-o", obj], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        res.update(kr.kernel_resources(obj))
    score = {name: r for name, r in res.items() if "score_" in name}
    assert sum("score_rows_kernel<" in name for name in score) == 4      # {32-, 64-bit index} x {segment grid, segment loop}
    assert any("score_rows_reduce_kernel" in name for name in score) and any("score_nodes_kernel" in name for name in score)
    for name, r in score.items():
        assert r["spill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 128, (name, r)
    count = [r for name, r in res.items() if "fit_count_kernel" in name]
    assert len(count) == 1 and count[0]["spill"] == 0 and count[0]["scratch"] == 0 and count[0]["lds"] == 4096 * 8
