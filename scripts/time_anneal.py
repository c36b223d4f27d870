"""Timing of simulated annealing as device-resident chains (bn_terms_create + bn_learn_anneal) on one MI355X against
the same chain driven from the host through what the library had before: one bn_learn_score_groups call per family term not yet
seen (memoised), the loop itself -- draws, cycle check, acceptance -- in Python (tests/anneal_refs.restated_chain).

Input: --draws forward samples of the ALARM-shaped network (tests/golden/alarm_shaped.dsc: 37 nodes, arities 2-4), q = 3, MDL,
the Metropolis rule, --schedule initial,final,rate.  Reported, not asserted, one JSON line: the term table's build time (device
events and host to host) and size; per chain count (1 / 64 / 1 024 / 8 192) the device time of the kernel (bn_learn_get
"anneal_ns"), host to host, iterations, device time per chain-step and chain-steps per second; the host-driven baseline for ONE
chain (host to host, device time of its score_groups calls, calls, time per step) and that the two ended in the same graph.
The device runs and the baseline alternate in one process, --reps times, warm; the best of each is reported.

  python scripts/time_anneal.py [--draws 2000] [--chains 1,64,1024,8192] [--schedule 20,0.5,0.99] [--reps 3] [--out FILE]
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
    ap.add_argument("--chains", default="1,64,1024,8192")
    ap.add_argument("--schedule", default="20,0.5,0.99")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    import anneal_refs as AR
    import learning_refs as LR
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable, score_groups

    t0, t1, rate = (float(x) for x in args.schedule.split(","))
    chain_counts = [int(x) for x in args.chains.split(",")]
    model, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    table = LR.sample_table(model, args.draws, 21)
    q, criterion = 3, "mdl"
    out = {"nodes": model.n, "patterns": int(table.pats.shape[0]), "samples": table.total, "max_parents": q, "schedule": [t0, t1, rate],
           "rule": "metropolis", "criterion": criterion}
    with InfoTable(table.pats, table.counts, model.k, device=0) as t:
        builds = []
        for _ in range(args.reps):
            h0 = time.perf_counter()
            with TermTable(t, q) as tt:
                builds.append((time.perf_counter() - h0, tt.info("build_ns") * 1e-9, tt.info("entries"), tt.info("families_scored")))
        out["term_table"] = {"host_s": min(b[0] for b in builds), "device_s": min(b[1] for b in builds), "entries": builds[0][2],
                             "families_scored": builds[0][3]}
        with TermTable(t, q) as tt:
            sched = AR.Schedule(t0, t1, rate, 1.0, 100, "metropolis")
            device = {c: [] for c in chain_counts}
            base = []
            for _ in range(args.reps):
                for c in chain_counts:
                    with Learner(t, None, criterion) as L:
                        h0 = time.perf_counter()
                        rec = L.anneal(tt, t0, t1, rate, chains=c, seed=args.seed, rule="metropolis")
                        device[c].append((time.perf_counter() - h0, L.info("anneal_ns") * 1e-9, int(rec["proposals"].sum()),
                                          [int(x) for x in rec["masks"][0]], float(rec["eval"].min())))
                # the baseline: chain 0, every family term through one score_groups call when first asked for
                memo, calls, dev_s = {}, 0, 0.0

                def term(child, parents):
                    nonlocal calls, dev_s
                    key = (child, tuple(parents))
                    if key not in memo:
                        memo[key] = score_groups(t, [(child, list(parents), [])])[0][0]
                        calls += 1
                        dev_s += (t.info("learn_count_ns") + t.info("learn_score_ns")) * 1e-9
                    return memo[key]

                pb = AR.Problem(table.k, q, criterion, table.total, term)
                h0 = time.perf_counter()
                r = AR.restated_chain(pb, sched, args.seed, 0)
                base.append((time.perf_counter() - h0, dev_s, calls, r["proposals"], r["masks"]))
            out["chains"] = {}
            for c in chain_counts:
                host, dev, steps, _, best = min(device[c])
                dev = min(x[1] for x in device[c])
                out["chains"][str(c)] = {"host_s": host, "device_s": dev, "chain_steps": steps, "device_ns_per_chain_step": dev * 1e9 / max(steps, 1),
                                         "chain_steps_per_s_device": steps / dev if dev else None, "chain_steps_per_s_host": steps / host,
                                         "best_eval": best}
            host, dev, calls, steps, masks = min(base)
            out["host_driven_one_chain"] = {"host_s": host, "device_s": dev, "score_groups_calls": calls, "chain_steps": steps,
                                            "host_us_per_chain_step": host * 1e6 / max(steps, 1),
                                            "same_graph_as_device_chain_0": masks == device[chain_counts[0]][0][3]}
            one = out["chains"][str(chain_counts[0])]
            out["one_chain_speedup_host_to_host"] = host / one["host_s"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
