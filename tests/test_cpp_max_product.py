"""bn::inference::max_product (include/bayesian/inference/max_product.hpp), the C++ face of bn_mpe_run: tests/cpp/test_max_product.cpp
is compiled by plain g++ against the stand-in data model of include/compat and the in-tree library and run on the GPU -- Pearl's
network with H = 0: mpe() equals the enumeration's assignment, operator() equals run() bit for bit, reload() sees an edited table --
and what it prints equals the Python result bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_max_product.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")


def build(tmp_path):
    exe = str(tmp_path / "test_max_product")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"), SRC,
           "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_max_product_header_compiles(bnlib, tmp_path):
    build(tmp_path)


@pytest.mark.gpu
def test_max_product_functor_on_pearl(bnlib, tmp_path):
    from bayesiannetwork_amd import Evidence, synth
    from bayesiannetwork_amd.engine import MaxProduct
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["failures"] == 0
    model = synth.pearl()
    mp = MaxProduct(model, device=0)
    try:
        ev = Evidence.from_dict(model, {3: 0})
        states, logp = mp.mpe(ev, 0.001, 50)
        assert d["states"] == states.tolist() and d["sweeps"] == mp.last["sweeps"]
        assert np.array_equal(np.asarray(d["max_marginals"]), mp.last["max_marginals"])   # (%.17g round-trips a double)
        assert d["log_probability"] == logp
        assert d["reloaded_states"] != d["states"]
    finally:
        mp.engine.close()
