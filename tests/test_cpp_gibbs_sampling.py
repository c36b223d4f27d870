"""bn::inference::gibbs_sampling (include/bayesian/inference/gibbs_sampling.hpp), the C++ face of bn_gibbs_run:
tests/cpp/test_gibbs_sampling.cpp is compiled by plain g++ against the stand-in data model of include/compat and the in-tree library
and run on the GPU -- Pearl's network with H = 0: operator() equals run() bit for bit, a second call runs fresh chains, reload() sees
an edited table -- and the marginals it prints equal GibbsSampling's bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_gibbs_sampling.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_gibbs_sampling")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"), SRC,
           "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_gibbs_sampling_header_compiles(bnlib, tmp_path):
    build(tmp_path)


@pytest.mark.gpu
def test_gibbs_sampling_functor_on_pearl(bnlib, tmp_path):
    from bayesiannetwork_amd import GibbsSampling, synth
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["failures"] == 0
    model = synth.pearl()
    gs = GibbsSampling(model, device=0, seed=12345)
    try:
        marg = gs({3: 0}, chains=256, sweeps=20, burn_in=5)
        assert np.array_equal(np.asarray(d["marginals"]), np.concatenate([np.ravel(x) for x in marg]))   # (%.17g round-trips a double)
        assert gs.last["kept"] == 256 * 15 and gs.last["states"].shape == (256, 4)
        assert d["reloaded_marginals"] != d["marginals"]
        cpt = np.asarray(model.cpt, dtype=np.float64).copy()
        cpt[0:2] = [0.9, 0.1]       # the edit of the C++ test: P(R)
        gs.engine.reload_cpt(cpt)
        gs._next = 0
        again = gs({3: 0}, chains=256, sweeps=20, burn_in=5)
        assert np.array_equal(np.asarray(d["reloaded_marginals"]), np.concatenate([np.ravel(x) for x in again]))
    finally:
        gs.engine.close()
