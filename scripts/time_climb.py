"""Timing of tabu hill climbing as device-resident runs (bn_terms_create + bn_learn_climb) on one MI355X, beside the
annealing chains over the same term table and a climb driven from the host through the public API: per step ONE
bn_learn_score_groups call for the candidate families of that step not yet seen (memoised), the loop itself -- legality, deltas,
the choice -- in Python (tests/climb_refs.climb_run).

Input: --draws forward samples of the ALARM-shaped network (tests/golden/alarm_shaped.dsc: 37 nodes, arities 2-4), q = 3, MDL,
--tabu tabu_len,max_worse, --perturb proposals per restart.  Reported, not asserted, one JSON line: the term table's build time;
per run count (1 / 4 096) the device time of the kernel (bn_learn_get "climb_ns"), host to host, applied steps, device time per
run and per step; the same for the annealing chains (--schedule, Metropolis) per chain and per iteration; the host-driven climb
for run 0 (host to host, score_groups calls, time per step) and that it ended in the graph of the device's run 0.
The device runs and the baseline alternate in one process, --reps times, warm; the best of each is reported.

  python scripts/time_climb.py [--draws 2000] [--runs 1,4096] [--tabu 10,10] [--perturb 20] [--schedule 20,0.5,0.99] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=2000)
    ap.add_argument("--runs", default="1,4096")
    ap.add_argument("--tabu", default="10,10")
    ap.add_argument("--perturb", type=int, default=20)
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--schedule", default="20,0.5,0.99")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import anneal_refs as AR
    import climb_refs as CR
    import learning_refs as LR
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable, score_groups

    tabu_len, max_worse = (int(x) for x in args.tabu.split(","))
    t0, t1, rate = (float(x) for x in args.schedule.split(","))
    run_counts = [int(x) for x in args.runs.split(",")]
    model, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    table = LR.sample_table(model, args.draws, 21)
    n, q, criterion = model.n, 3, "mdl"
    out = {"nodes": n, "patterns": int(table.pats.shape[0]), "samples": table.total, "max_parents": q, "criterion": criterion,
           "tabu_len": tabu_len, "max_worse": max_worse, "perturb": args.perturb, "max_steps": args.max_steps, "schedule": [t0, t1, rate]}
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        h0 = time.perf_counter()
        with TermTable(t, q) as tt:
            out["term_table"] = {"host_s": time.perf_counter() - h0, "device_s": tt.info("build_ns") * 1e-9, "entries": tt.info("entries")}
            climb = {c: [] for c in run_counts}
            anneal = {c: [] for c in run_counts}
            base = []
            for _ in range(args.reps):
                for c in run_counts:
                    with Learner(t, None, criterion) as L:
                        h0 = time.perf_counter()
                        rec = L.climb(tt, tabu_len, max_worse, c, args.perturb, args.seed, max_steps=args.max_steps)
                        climb[c].append((time.perf_counter() - h0, L.info("climb_ns") * 1e-9, int(rec["steps"].sum()),
                                         [int(x) for x in rec["masks"][0]], float(rec["score"].min())))
                    with Learner(t, None, criterion) as L:
                        h0 = time.perf_counter()
                        rec = L.anneal(tt, t0, t1, rate, chains=c, seed=args.seed, rule="metropolis")
                        anneal[c].append((time.perf_counter() - h0, L.info("anneal_ns") * 1e-9, int(rec["proposals"].sum()), float(rec["eval"].min())))
                # the baseline: run 0; before every look at the moves the candidate families not yet seen go through ONE score_groups call
                memo, calls = {}, 0

                class Row:
                    def __init__(self, c):
                        self.c = c

                    def __getitem__(self, r):
                        return memo[(self.c, r)]

                def prefetch(parents):
                    nonlocal calls
                    want = {}
                    for to in range(n):
                        fams = [tuple(parents[to])] + [tuple(u for u in parents[to] if u != frm) for frm in parents[to]]
                        if len(parents[to]) < q:
                            fams += [tuple(sorted(parents[to] + [frm])) for frm in range(n) if frm != to and frm not in parents[to]]
                        for S in fams:
                            key = (to, AR.rank(n, to, S))
                            if key not in memo:
                                want[key] = (to, list(S), [])
                    if want:
                        for key, ll in zip(want, score_groups(t, list(want.values()))):
                            memo[key] = ll[0]
                        calls += 1

                pb = CR.Problem(table.k, q, criterion, table.total, [Row(c) for c in range(n)])
                pb.prefetch = prefetch
                h0 = time.perf_counter()
                prefetch(pb.start)
                r = CR.climb_run(pb, tabu_len, max_worse, args.max_steps, args.perturb, args.seed, 0)
                base.append((time.perf_counter() - h0, calls, r["steps"], r["masks"]))
            out["climb"], out["anneal"] = {}, {}
            for c in run_counts:
                host, _, steps, _, best = min(climb[c])
                dev = min(x[1] for x in climb[c])
                out["climb"][str(c)] = {"host_s": host, "device_s": dev, "steps": steps, "device_us_per_run": dev * 1e6 / c,
                                        "device_ns_per_step": dev * 1e9 / max(steps, 1), "best_score": best}
                host, _, steps, best = min(anneal[c])
                dev = min(x[1] for x in anneal[c])
                out["anneal"][str(c)] = {"host_s": host, "device_s": dev, "iterations": steps, "device_us_per_chain": dev * 1e6 / c,
                                         "device_ns_per_iteration": dev * 1e9 / max(steps, 1), "best_eval": best}
            host, calls, steps, masks = min(base)
            out["host_driven_run_0"] = {"host_s": host, "score_groups_calls": calls, "steps": steps, "host_us_per_step": host * 1e6 / max(steps, 1),
                                        "same_graph_as_device_run_0": masks == climb[run_counts[0]][0][3]}
            out["run_0_speedup_host_to_host"] = host / out["climb"][str(run_counts[0])]["host_s"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
