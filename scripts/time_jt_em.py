"""Timing of the exact E-step (bn_jt_em_expected_counts: the junction tree, one workgroup per row) on one MI355X next to the
belief-propagation E-step (bn_em_expected_counts) over the same rows, in the same process on the same engine.

  network   tests/golden/alarm_shaped.dsc (37 nodes)
  table     --rows distinct forward samples of the network (default 4 096) with --missing of the cells blanked (default 25 %), count 1
            (scripts/time_em.py's table)
  exact     bn_get_info "jt_em_estep_ns": device events around the E-step's kernels -- the base potentials of the tables, one
            jt_em_kernel launch per chunk of rows with the accumulating kernel behind it, the log-likelihood's sum
  BP        bn_get_info "em_estep_ns" of bn_em_expected_counts(bp_eps, cap): the same brackets around its kernels
The host clock around each whole call (table upload included) is reported beside the device times.  After --warmup untimed rounds the
two sides alternate --reps times; median, quartiles, minimum and maximum of each, and the ratio of the medians.  Also the largest
difference of the two E results: what loopy belief propagation is off by on this table.  One JSON object on stdout (and into --out).
Needs a GPU: there is no CPU path.

  python scripts/time_jt_em.py [--rows 4096] [--missing 0.25] [--reps 10] [--warmup 3] [--eps 1e-3] [--cap 100] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_em import distinct_rows, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--missing", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.engine import Engine

    model = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    pats = distinct_rows(model, args.rows, args.missing, seed=17)
    counts = np.ones(args.rows, dtype=np.uint64)
    S = int(model.cpt_off[-1])
    exact, exact_host, bp, bp_host = [], [], [], []
    with Engine(model, device=0) as eng:
        assert eng.info("jt_eligible") == 1 and eng.info("em_eligible") == 1
        plan = eng.jt_plan()
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            E, ll = eng.jt_em_expected_counts(pats, counts)
            t1 = time.perf_counter()
            x_ns = eng.info("jt_em_estep_ns")
            t2 = time.perf_counter()
            E_bp, sweeps = eng.em_expected_counts(pats, counts, args.eps, args.cap)
            t3 = time.perf_counter()
            b_ns = eng.info("em_estep_ns")
            if rep < args.warmup:
                continue
            exact.append(x_ns * 1e-3)
            exact_host.append((t1 - t0) * 1e6)
            bp.append(b_ns * 1e-3)
            bp_host.append((t3 - t2) * 1e6)
        form, launches, skipped = eng.info("jt_em_last_form"), eng.info("jt_em_last_launches"), eng.info("jt_em_skipped")
    sx, sb = summary(exact), summary(bp)
    rec = {"network": "alarm_shaped", "rows": args.rows, "missing": args.missing, "entries": S, "cliques": plan["cliques"],
           "state_cells": plan["state_cells"], "form": form, "launches": launches, "skipped_families": skipped,
           "loglik": float(ll.sum()), "exact_estep_device_us": sx, "exact_estep_ns_per_row": sx["median"] * 1e3 / args.rows,
           "exact_call_host_us": summary(exact_host), "bp_eps": args.eps, "bp_cap": args.cap, "bp_sweeps_total": int(sweeps.sum()),
           "bp_estep_device_us": sb, "bp_estep_ns_per_row": sb["median"] * 1e3 / args.rows, "bp_call_host_us": summary(bp_host),
           "exact_over_bp": sx["median"] / sb["median"], "max_abs_E_difference": float(np.abs(E - E_bp).max()),
           "b_bytes_written_and_read": 2 * 8 * S * args.rows}
    text = json.dumps(rec)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
