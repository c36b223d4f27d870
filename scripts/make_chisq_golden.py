"""Writes tests/golden/chisq_sf.json: the chi-square upper tail Q(df / 2, G / 2) to 50 significant digits over the grid of
tests/ci_refs.golden_grid, computed with mpmath at 80 digits.  Run once, by hand, where mpmath is installed; the tests read the JSON
only.  A tail below 1e-100000 is written as "0"."""
import json
import os
import sys

import mpmath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ci_refs  # noqa: E402


def main():
    mpmath.mp.dps = 80
    rows = []
    for df, g in ci_refs.golden_grid():
        a, x = mpmath.mpf(df) / 2, mpmath.mpf(g) / 2     # (g is a double: exact in mpf)
        q = mpmath.mpf(1) if g == 0.0 else mpmath.gammainc(a, x, mpmath.inf, regularized=True)
        text = "0" if q < mpmath.mpf(10) ** -100000 else mpmath.nstr(q, 50, min_fixed=0, max_fixed=0)
        rows.append({"df": df, "g": float(g).hex(), "sf": text})
        print(df, g, text, flush=True)
    with open(os.path.join(ROOT, "tests", "golden", "chisq_sf.json"), "w") as f:
        json.dump({"digits": 50, "rows": rows}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
