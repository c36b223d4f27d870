"""Timing of constraint-based structure learning (bn_learn_pc) on one MI355X, beside the same learning done through
what the library offered before it: per level ONE bn_learn_score_groups call for the groups "child x, base S, candidates y", G^2 as
2 (ll(x | S + y) - ll(x | S)), the nominal degrees of freedom and the chi-square tail on the host (tests/ci_refs.chisq_sf), the
level loop, the separating sets and the orientation in Python (tests/pc_refs.pc_stable).

Input: --draws forward samples of the ALARM-shaped network (tests/golden/alarm_shaped.dsc: 37 nodes, arities 2-4), --alpha,
--max-cond.  Reported, not asserted, one JSON line: per level the number of tests and the device time of the counting and the
statistic kernels; the whole call host to host, device-driven and host-driven; each as median and range over --reps warm
repetitions, the two alternating in one process; and whether both ended in the same CPDAG.

  python scripts/time_pc.py [--draws 2000] [--alpha 0.05] [--max-cond 3] [--reps 5] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=2000)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--max-cond", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np

    import ci_refs as C
    import learning_refs as LR
    import pc_refs as P
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import PC, score_groups

    model, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    table = LR.sample_table(model, args.draws, 21)
    k = [int(x) for x in table.k]
    out = {"nodes": model.n, "patterns": int(table.pats.shape[0]), "samples": table.total, "alpha": args.alpha, "max_cond": args.max_cond,
           "reps": args.reps}
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        calls = []

        def host_p_values(tests):
            groups = {}
            for x, y, S in tests:
                groups.setdefault((x, tuple(S)), []).append(y)
            h0 = time.perf_counter()
            lls = score_groups(t, [(x, list(S), ys) for (x, S), ys in groups.items()])
            calls.append((len(tests), time.perf_counter() - h0, t.info("learn_count_ns") * 1e-9, t.info("learn_score_ns") * 1e-9))
            p = {}
            for ((x, S), ys), ll in zip(groups.items(), lls):
                strata = math.prod(k[v] for v in S)
                for y, lly in zip(ys, ll[1:]):
                    g = 2.0 * (lly - ll[0])
                    p[(x, y, S)] = C.chisq_sf(g if g > 0.0 else 0.0, (k[x] - 1) * (k[y] - 1) * strata)
            return [p[(x, y, tuple(S))] for x, y, S in tests]

        dev, host = [], []
        PC(args.alpha, args.max_cond)(t)   # (the first call of a process also loads the code objects)
        for _ in range(args.reps):
            h0 = time.perf_counter()
            r = PC(args.alpha, args.max_cond)(t)
            dev.append((time.perf_counter() - h0, r))
            calls.clear()
            h0 = time.perf_counter()
            w = P.pc_stable(k, host_p_values, args.alpha, args.max_cond)
            host.append((time.perf_counter() - h0, w, list(calls)))
        n_levels = len(dev[0][1].levels)
        out["device_driven"] = {
            "host_s": spread([d[0] for d in dev]),
            "levels": [{"tests": dev[0][1].levels[l]["tests"], "removed": dev[0][1].levels[l]["removed"],
                        "count_us": spread([d[1].levels[l]["count_ns"] * 1e-3 for d in dev]),
                        "stat_us": spread([d[1].levels[l]["stat_ns"] * 1e-3 for d in dev])} for l in range(n_levels)]}
        out["host_driven"] = {
            "host_s": spread([h[0] for h in host]),
            "levels": [{"tests": host[0][2][l][0], "score_groups_s": spread([h[2][l][1] for h in host]),
                        "count_us": spread([h[2][l][2] * 1e6 for h in host]), "score_us": spread([h[2][l][3] * 1e6 for h in host])}
                       for l in range(len(host[0][2]))]}
        out["same_cpdag"] = bool(np.array_equal(dev[0][1].cpdag, host[0][1]["cpdag"]))
        out["speedup_host_to_host"] = out["host_driven"]["host_s"]["median"] / out["device_driven"]["host_s"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
