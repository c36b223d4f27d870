#!/usr/bin/env python3
"""Randomised parity soak on the GPU box, for long runs on a free machine:
    python scripts/soak_gpu.py [seconds] [seed] [--leg bp|tables]     cases 0, 1, ... of that seed until the budget is spent
    python scripts/soak_gpu.py --case leg:seed:index                  one case, e.g. the one a failure of tests/test_soak_gpu.py names
The cases and their comparisons are tests/soak_cases.py's (leg `bp`: random networks x evidence x eps through every
belief-propagation path against the oracle; leg `tables`: random pattern tables through the table kernels against the host
references); tests/test_soak_gpu.py runs a fixed number of them in the GPU suite.  A case is a function of its key, so --case
replays exactly the comparison that failed.  Prints one line per case and a summary; exits non-zero on the first difference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import soak_cases  # noqa: E402

if __name__ == "__main__":
    sys.exit(soak_cases.soak_main(sys.argv[1:], ("bp", "tables"), "bp", soak_cases.SUITE["bp"]["seed"]))
