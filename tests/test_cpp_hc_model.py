"""CPU: tests/cpp/test_hc.cpp -- and with it include/bayesian/learning/stepwise_structure_hc.hpp and the headers it pulls in --
compiles over both data models: this repository's stand-in (include/compat) and the reference's own graph.hpp / sampler.hpp, where
the reference's headers are (the directory oracle/Makefile names as REF, or the environment's REF).  Syntax only: nothing is
linked or run."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hc.cpp")


def reference_dir():
    if os.environ.get("REF"):
        return os.environ["REF"]
    m = re.search(r"^REF\s*\?=\s*(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return m.group(1) if m else ""


def syntax_only(model_dir):
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", model_dir, SRC]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]


def test_the_hc_header_compiles_over_the_stand_in_model():
    syntax_only(os.path.join(ROOT, "include", "compat"))


def test_the_hc_header_compiles_over_the_reference_model():
    ref = reference_dir()
    if not os.path.exists(os.path.join(ref, "bayesian", "graph.hpp")):
        pytest.skip("the reference's headers are not on this machine")
    syntax_only(ref)
