"""Timing of the exact structure search (bn_terms_create + bn_learn_optimal) on one MI355X, beside the numpy
restatement (tests/optimal_refs.py) and the tabu climb over the same term table.

Input: --draws forward samples of the ALARM-shaped network (tests/golden/alarm_shaped.dsc), its first n columns for every n of
--nodes (default 16, 20, 24), q = 3, MDL.  Reported, not asserted, one JSON line.  Per n: the device time of the whole call
(bn_learn_get "optimal_ns") and of its steps -- the best-parent-set passes ("optimal_bps_ns"), the best-sink levels
("optimal_sink_ns") and the walk back (the rest) -- over --reps calls after --warmup, as median, min and max; host to host; the
bytes step 1 moves (12 per cell written by the first pass, 24 per cell read and written by every later one) and the rate that
makes, against the better of the library's copy / triad kernels (bn_debug_stream); `--climb-runs` tabu climbs on the same table:
device time, and the gap between the best climb's score and the optimum's.  At --restate-nodes (default 16) also the restatement's
host time, and that it gives the device's graph.

  python scripts/time_optimal.py [--nodes 16,20,24] [--draws 2000] [--reps 7] [--warmup 2] [--climb-runs 4096] [--out FILE]
"""
import argparse
import ctypes
import json
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
    ap.add_argument("--nodes", default="16,20,24")
    ap.add_argument("--draws", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--climb-runs", type=int, default=4096)
    ap.add_argument("--restate-nodes", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    import learning_refs as LR
    import optimal_refs as OR
    from bayesiannetwork_amd import _lib
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import Learner, TermTable

    model, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    full = LR.sample_table(model, args.draws, 21)
    q, criterion = 3, "mdl"
    stream = 0.0
    for mode in (0, 1):
        g = ctypes.c_double()
        _lib.check(_lib.lib().bn_debug_stream(0, mode, 1 << 30, 5, ctypes.byref(g)))
        stream = max(stream, g.value)
    out = {"max_parents": q, "criterion": criterion, "samples": full.total, "reps": args.reps, "warmup": args.warmup,
           "stream_gbs": stream, "sizes": {}}
    for n in (int(x) for x in args.nodes.split(",")):
        pats, k = full.pats[:, :n], full.k[:n]
        rec = {}
        with InfoTable(pats, full.counts, k, device=0) as t, TermTable(t, q, criterion) as tt:
            rec["term_table_device_s"] = tt.info("build_ns") * 1e-9
            total, bps, sink, host = [], [], [], []
            for i in range(args.warmup + args.reps):
                with Learner(t, None, criterion) as L:
                    h0 = time.perf_counter()
                    got = L.optimal(tt)
                    h1 = time.perf_counter()
                    if i >= args.warmup:
                        total.append(L.info("optimal_ns") * 1e-9)
                        bps.append(L.info("optimal_bps_ns") * 1e-9)
                        sink.append(L.info("optimal_sink_ns") * 1e-9)
                        host.append(h1 - h0)
                    cells, nbytes, score = L.info("optimal_cells"), L.info("optimal_bytes"), L.score()
            m = n - 1
            passes = 1 if m <= 12 else 1 + (m - 12 + 7) // 8
            moved = cells * 12 * (1 + 2 * (passes - 1))
            rec.update({"cells": cells, "bytes": nbytes, "device_s": spread(total), "step1_s": spread(bps), "step2_s": spread(sink),
                        "step3_s": spread([a - b - c for a, b, c in zip(total, bps, sink)]), "host_s": spread(host),
                        "step1_passes": passes, "step1_bytes_moved": moved, "step1_gbs": moved / statistics.median(bps) * 1e-9,
                        "step1_share_of_stream": moved / statistics.median(bps) * 1e-9 / stream, "value": got["value"], "score": score})
            with Learner(t, None, criterion) as L:
                h0 = time.perf_counter()
                runs = L.climb(tt, 10, 10, args.climb_runs, 20, 1, max_steps=1000)
                rec["climb"] = {"runs": args.climb_runs, "host_s": time.perf_counter() - h0, "device_s": L.info("climb_ns") * 1e-9,
                                "best_score": L.score(), "gap_to_optimum": L.score() - score,
                                "runs_at_optimum": int((runs["score"] <= score + OR.margin(n, abs(score))).sum())}
            if n == args.restate_nodes:
                rows = [tt.row(c) for c in range(n)]
                pb = OR.Problem(k, q, criterion, full.total, rows)
                h0 = time.perf_counter()
                want = OR.optimal(pb)
                rec["restatement"] = {"host_s": time.perf_counter() - h0, "same_graph": want["masks"] == [int(x) for x in got["masks"]]}
        out["sizes"][str(n)] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
