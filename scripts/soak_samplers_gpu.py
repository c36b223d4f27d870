#!/usr/bin/env python3
"""Randomised parity soak of the sampler family on the GPU box, for long runs on a free machine:
    python scripts/soak_samplers_gpu.py [seconds] [seed]              cases 0, 1, ... of that seed until the budget is spent
    python scripts/soak_samplers_gpu.py --case samplers:seed:index    one case
The cases and their comparisons are the `samplers` leg of tests/soak_cases.py (random DAGs of arities 1 ... 8 and up to 6 parents x
hard evidence x sample counts, seeds and offsets: states bit-equal to the oracle's, weights <= 1e-12, the weighted histogram
<= 1e-9, rejection sampling exact, CPT fitting bit-equal); tests/test_soak_gpu.py runs a fixed number of them in the GPU suite."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import soak_cases  # noqa: E402

if __name__ == "__main__":
    sys.exit(soak_cases.soak_main(sys.argv[1:], ("samplers",), "samplers", soak_cases.SUITE["samplers"]["seed"]))
