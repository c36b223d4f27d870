"""Timing of the Bayesian-Dirichlet family term (bn_learn_score_groups_spec, kind 2) on one MI355X against the log-likelihood term
(kind 0) of the SAME batch of families, and of one greedy structure under either.

Shapes: --draws forward samples of the ALARM-shaped network (tests/golden/alarm_shaped.dsc: 37 columns, arities 2-4).  The batch is
what a greedy pass offers: per child one group with no base parent and every other node as a candidate (37 groups, 37 * 37
families).  The two kinds are timed in one process, alternating, --reps times, warm; the best of each is reported: the device time
of the scoring launch and of the counting launch (bn_info_get "learn_score_ns" / "learn_count_ns": device events) and host to
host.  Then one greedy structure (fixed orders, max_parents 6) under "mdl" and under "bdeu": host to host and the learner's summed
device times.  One JSON line.

  python scripts/time_bd.py [--draws 20000] [--reps 5] [--ess 1.0] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sample_table(model, draws, seed):
    """Forward samples by ancestral order of the node ids (a parent with a larger id is read at state 0), equal rows merged."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((draws, model.n), dtype=np.uint8)
    for v in range(model.n):
        ps = model.parents(v)
        row = np.zeros(draws, dtype=np.int64)
        for u in ps:
            row = row * int(model.k[u]) + (rows[:, u] if u < v else 0)
        cpt = model.cpt[model.cpt_off[v]:model.cpt_off[v + 1]].reshape(-1, int(model.k[v]))
        cum = np.cumsum(cpt[row], axis=1)
        rows[:, v] = np.minimum((rng.random(draws)[:, None] * cum[:, -1:] > cum).sum(axis=1), int(model.k[v]) - 1)
    pats, counts = np.unique(rows, axis=0, return_counts=True)
    return pats, counts.astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ess", type=float, default=1.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.evaluation import BDeu, InfoTable
    from bayesiannetwork_amd.learning import Learner, score_groups
    model, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    pats, counts = sample_table(model, a.draws, 1)
    n = model.n
    groups = [(c, [], [u for u in range(n) if u != c]) for c in range(n)]
    kinds = {"loglik": "mdl", "bdeu": BDeu(a.ess)}
    rng = np.random.default_rng(2)
    children = [int(v) for v in rng.permutation(n)]
    tails = [[children[j] for j in i + 1 + rng.permutation(n - i - 1)] for i in range(n)]
    out = {"what": "time_bd", "patterns": int(len(counts)), "draws": a.draws, "families": n * n, "ess": a.ess, "reps": a.reps}
    with InfoTable(pats, counts, model.k, device=0) as t:
        for crit in kinds.values():
            score_groups(t, groups, criterion=crit)   # warm
        best = {name: {"score_ns": float("inf"), "count_ns": float("inf"), "host_s": float("inf")} for name in kinds}
        for _ in range(a.reps):
            for name, crit in kinds.items():
                t0 = time.perf_counter()
                score_groups(t, groups, criterion=crit)
                host = time.perf_counter() - t0
                b = best[name]
                b["score_ns"] = min(b["score_ns"], t.info("learn_score_ns"))
                b["count_ns"] = min(b["count_ns"], t.info("learn_count_ns"))
                b["host_s"] = min(b["host_s"], host)
        out["batch"] = best
        out["score_launch_ratio_bdeu_over_loglik"] = best["bdeu"]["score_ns"] / max(best["loglik"]["score_ns"], 1.0)
        out["greedy"] = {}
        for name, crit in kinds.items():
            runs = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                with Learner(t, None, crit, 6) as L:
                    for child, tail in zip(children, tails):
                        L.try_parents(child, tail)
                    runs.append({"host_s": time.perf_counter() - t0, "edges": L.info("edges"), "passes": L.info("passes"),
                                 "count_ns": L.info("count_ns"), "score_ns": L.info("score_ns"), "score": L.score()})
            out["greedy"][name] = min(runs, key=lambda r: r["host_s"])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
