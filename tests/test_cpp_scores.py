"""bn::evaluation::aic / mdl of the C++ drop-in (include/bayesian/evaluation/aic.hpp, mdl.hpp, compiled over include/compat
like tests/cpp/test_dropin.cpp) against the Python functors -- bit for bit -- and against the restatement of the reference's
loop (tests/loglik_refs.py reference_aic / reference_mdl) to the order-free bound gamma_m x sum |terms|."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import exact_refs
import loglik_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_scores.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")
ALARM = os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc")


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_scores")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           SRC, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def sampled_table(model, draws, seed):
    """{pattern: count} of `draws` forward samples (only patterns the network can produce: pearl's CPTs hold zeros)"""
    rng = np.random.default_rng(seed)
    table = {}
    for _ in range(draws):
        key = tuple(int(x) for x in exact_refs.forward_sample(model, rng))
        table[key] = table.get(key, 0) + int(rng.integers(1, 50))
    return table


def score_bound(model, table, nodes, extra):
    """gamma_m x sum |terms| over everything the score adds: the non-zero count x log terms of `nodes`, and `extra`
    (the parameter term); m = their number + 1."""
    pats = np.array(list(table.keys()), dtype=np.uint8)
    N = R.family_counts_ref(model, pats, np.array(list(table.values()), dtype=np.uint64))
    L = R.log_table(model)
    mags, m = [abs(extra)], 1
    for v in nodes:
        t = R.node_terms(model, N, L, v)
        t = t[t != 0]
        m += len(t)
        mags.extend(np.abs(t).tolist())
    return R.gamma(m + 1) * math.fsum(mags)


@pytest.mark.parametrize("net", ["pearl", "alarm"])
def test_cpp_functors_equal_python_and_the_reference_loop(bnlib, tmp_path, net):
    from bayesiannetwork_amd import AIC, MDL, synth
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.engine import Engine, Sampler
    from bayesiannetwork_amd.evaluation import InfoTable, log_likelihood_nodes, log_likelihood_rows
    model = synth.pearl() if net == "pearl" else load_dsc(ALARM)[0]
    table = sampled_table(model, 400, seed=21)
    path = tmp_path / "samples.txt"
    path.write_text("".join(f"{c} " + " ".join(str(s) for s in key) + "\n" for key, c in table.items()))
    exe = build_cpp(tmp_path)
    args = [exe, "--pearl", str(path)] if net == "pearl" else [exe, "--dsc", ALARM, str(path)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads(out.stdout)
    size = sum(table.values())
    assert d["n"] == model.n and d["sampling_size"] == size

    sampler = Sampler()
    sampler.load_sample(table)
    subset = [i for i in range(model.n - 1, -1, -1) if i % 2 == 1]
    aic, mdl = AIC(sampler, device=0), MDL(sampler, device=0)
    with Engine(model, device=0) as eng:
        py = {"aic": aic(eng), "mdl": mdl(eng), "aic_subset": aic(eng, subset), "mdl_subset": mdl(eng, subset)}
        assert aic(model) == py["aic"] and mdl(model, subset) == py["mdl_subset"]      # a model in place of an engine
        # Python and C++: the same kernels in the same order, the same host arithmetic -- equal bit for bit
        for key, want in py.items():
            print(f"{net} {key}: python {want!r} c++ {d[key]!r} reference {(R.reference_aic if 'aic' in key else R.reference_mdl)(model, table, subset if 'subset' in key else None)!r}")
            assert d[key] == want, key
        assert d["aic_again"] == d["aic"]
        # the C++ table's row order is the hash map's: compare per pattern
        pats = np.array(d["row_patterns"], dtype=np.uint8)
        cnts = np.array([table[tuple(r)] for r in pats.tolist()], dtype=np.uint64)
        with InfoTable(pats, cnts, model.k, device=0) as t:
            assert np.array_equal(np.array([float(x) for x in d["ll_rows"]]), log_likelihood_rows(eng, t))
            assert np.array_equal(np.array([float(x) for x in d["ll_node"]]), log_likelihood_nodes(eng, t))
    # against the reference's loop, whose order of additions is its hash map's: to the order-free bound
    params = float(R.parameters_ref(model))
    corr = math.log2(size) / 2
    for key, nodes, ref, extra in (("aic", range(model.n), R.reference_aic(model, table), params),
                                   ("aic_subset", subset, R.reference_aic(model, table, subset), params),
                                   ("mdl", range(model.n), R.reference_mdl(model, table), params * corr),
                                   ("mdl_subset", subset, R.reference_mdl(model, table, subset), params * corr)):
        bound = score_bound(model, table, nodes, extra)
        print(f"{net} {key}: |got - reference| = {abs(py[key] - ref):.3e}, bound {bound:.3e}")
        assert math.isfinite(ref) and abs(py[key] - ref) <= bound, key
    # a node subset keeps the whole graph's parameters
    with Engine(model, device=0) as eng:
        assert aic(eng, []) == params and mdl(eng, []) == params * corr
    assert d["empty_aic"] == params and d["empty_mdl_throws"] is True
    with pytest.raises(RuntimeError, match="Sampling is not finished yet."):
        MDL(Sampler())(model)
    assert AIC(Sampler())(model) == params
