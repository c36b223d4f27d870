"""Timing of the hierarchical-clustering structure search as device-resident runs (bn_terms_create + bn_learn_hc) on
one MI355X, beside two searches the library already had on the same tables: StepwiseStructure(inner=Greedy, between=Greedy,
initial_cluster_size=1) and SimulatedAnnealing.

Inputs: the 37-node `alarm2k_mdl` table of tests/learning_refs.py (2 000 forward samples of tests/golden/alarm_shaped.dsc, MDL,
q = 3) and `n64` of tests/anneal_refs.py (64 binary nodes, 2 049 samples, MDL, q = 2).  Reported, not asserted, one JSON line per
table: the term table's build time (device events and host to host); per run count (1 / 64 / 1 024 / 4 096) the device time of the
kernel (bn_learn_get "hc_ns"), host to host, runs per second and the best score reached; StepwiseStructure: ms per search (host
to host) and its score; SimulatedAnnealing (Metropolis, 20 -> 0.5 at 0.95): device ms per chain and its best score.  Warm, the
best of --reps.

  python scripts/time_hc.py [--runs 1,64,1024,4096] [--alpha 0.3] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="1,64,1024,4096")
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import anneal_refs as AR
    import learning_refs as LR
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Greedy, Learner, SimulatedAnnealing, StepwiseStructure, TermTable, structure_model

    run_counts = [int(x) for x in args.runs.split(",")]
    model, table, _, _, _ = LR.learning_input("alarm2k_mdl")
    _, table64 = AR.anneal_input("n64")
    lines = []
    for name, tab, q in (("alarm2k_mdl", table, 3), ("n64", table64, 2)):
        out = {"table": name, "nodes": tab.n, "patterns": int(tab.pats.shape[0]), "samples": tab.total, "max_parents": q,
               "criterion": "mdl", "alpha": args.alpha}
        start = structure_model(tab.k, np.zeros(tab.n + 1, np.int32), np.zeros(0, np.int32))
        with InfoTable(tab.pats, tab.counts, tab.k, device=0) as t:
            builds = []
            for _ in range(args.reps):
                h0 = time.perf_counter()
                with TermTable(t, q) as tt:
                    builds.append((time.perf_counter() - h0, tt.info("build_ns") * 1e-9, tt.info("entries")))
            out["term_table"] = {"host_ms": min(b[0] for b in builds) * 1e3, "device_ms": min(b[1] for b in builds) * 1e3, "entries": builds[0][2]}
            with Learner(t, None, "mdl") as L0:
                out["empty_score"] = L0.score()
            with TermTable(t, q) as tt:
                out["hc"] = {}
                for runs in run_counts:
                    best = None
                    for _ in range(args.reps):
                        with Learner(t, None, "mdl") as L:
                            h0 = time.perf_counter()
                            rec = L.hc(tt, args.alpha, runs, args.seed)
                            host = time.perf_counter() - h0
                            dev = L.info("hc_ns") * 1e-9
                            row = (dev, host, float(rec["score"].min()), int(rec["merges"].sum()), int(rec["tried"].sum()))
                            best = row if best is None or row < best else best
                    dev, host, score, merges, tried = best
                    out["hc"][str(runs)] = {"kernel_ms": dev * 1e3, "host_ms": host * 1e3, "runs_per_s": runs / dev if dev else None,
                                            "best_score": score, "merges": merges, "candidates_evaluated": tried}
            best = None
            for rep in range(args.reps):
                sw = StepwiseStructure("mdl", t, inner=Greedy, between=Greedy, seed=args.seed + rep, max_parents=q)
                h0 = time.perf_counter()
                _, score = sw(start, 1)
                row = (time.perf_counter() - h0, score)
                best = row if best is None or row < best else best
            out["stepwise_structure_greedy"] = {"ms_per_search": best[0] * 1e3, "score": best[1]}
            best = None
            for rep in range(args.reps):
                sa = SimulatedAnnealing("mdl", t, max_parents=q, chains=64, rule="metropolis", seed=args.seed + rep)
                _, score = sa(start, 20.0, 0.5, 0.95)
                row = (sa.last["anneal_ns"] * 1e-6 / 64, score, sa.last["anneal_ns"] * 1e-6)
                best = row if best is None or row < best else best
                sa.close()
            out["simulated_annealing_64_chains"] = {"kernel_ms_per_chain": best[0], "kernel_ms": best[2], "score": best[1]}
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
