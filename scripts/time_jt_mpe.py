"""Timing of exact MPE on the junction tree (bn_jt_mpe_*) on one MI355X next to the sum run of the same tree (bn_jt_*) and to
max-product belief propagation (bn_mpe_run), in the same process on the same library.  A record, not a gate.

  single   tests/golden/alarm_shaped.dsc (37 nodes, 27 cliques, state in LDS), 10 % hard evidence: one bn_jt_mpe_run, one bn_jt_run
           and one bn_mpe_run at --eps, alternating.  Per call the host clock around it (the call synchronises); for the two
           junction-tree runs also the device time between HIP events around the launch (option "timing", bn_get_info
           "jt_last_kernel_ns").  The comparison value of the max run is the sum run of the same session.
  batch    256 evidence sets on the same network: bn_jt_mpe_run_batch against bn_jt_run_batch.
After --warmup untimed rounds the sides alternate --reps times; median, quartiles, minimum and maximum of each are reported.
One JSON object on stdout (and into --out).  Needs a GPU: there is no CPU path.

  python scripts/time_jt_mpe.py [--reps 30] [--warmup 5] [--eps 1e-3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(xs):
    a = np.sort(np.asarray(xs, dtype=np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median": float(med), "q1": float(q1), "q3": float(q3), "min": float(a[0]), "max": float(a[-1]), "n": int(a.size)}


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from bayesiannetwork_amd import synth
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.engine import Engine

    alarm = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    ev = synth.random_evidence(alarm, 0.1, seed=7)
    sets = [synth.random_evidence(alarm, 0.1 + 0.2 * (q % 2), seed=100 + q) for q in range(256)]
    names = ("jt_mpe_host", "jt_mpe_dev", "jt_host", "jt_dev", "mpe_host", "jt_mpe_b_host", "jt_mpe_b_dev", "jt_b_host", "jt_b_dev")
    t = {k: [] for k in names}
    # one engine per side, as scripts/time_jtree.py: no side pays for the other's buffers
    with Engine(alarm, device=0) as mx, Engine(alarm, device=0) as jt, Engine(alarm, device=0) as bp:
        mx.set_option("timing", 1)
        jt.set_option("timing", 1)
        for rep in range(args.warmup + args.reps):
            a, ra = clock(lambda: mx.jt_mpe_run(ev))
            a_dev = mx.info("jt_last_kernel_ns") * 1e-3
            b, _ = clock(lambda: jt.jt_run(ev))
            b_dev = jt.info("jt_last_kernel_ns") * 1e-3
            c, rc = clock(lambda: bp.mpe_run(ev, args.eps))
            d, _ = clock(lambda: mx.jt_mpe_run_batch(sets))
            d_dev = mx.info("jt_last_kernel_ns") * 1e-3
            e, _ = clock(lambda: jt.jt_run_batch(sets))
            e_dev = jt.info("jt_last_kernel_ns") * 1e-3
            if rep >= args.warmup:
                for k, x in zip(names, (a, a_dev, b, b_dev, c, d, d_dev, e, e_dev)):
                    t[k].append(x)
        rec = {"eps": args.eps, "cliques": mx.info("jt_cliques"), "levels": mx.info("jt_levels"), "state_cells": mx.info("jt_state_cells"),
               "form": mx.info("jt_last_form"), "mpe_sweeps": rc["sweeps"], "mpe_converged": bool(rc["converged"]),
               "states_agree_with_max_product": bool(np.array_equal(ra["states"], rc["states"])),
               "jt_mpe_run_host_us": summary(t["jt_mpe_host"]), "jt_mpe_run_device_us": summary(t["jt_mpe_dev"]),
               "jt_run_host_us": summary(t["jt_host"]), "jt_run_device_us": summary(t["jt_dev"]),
               "mpe_run_host_us": summary(t["mpe_host"]),
               "jt_mpe_batch256_host_us": summary(t["jt_mpe_b_host"]), "jt_mpe_batch256_device_us": summary(t["jt_mpe_b_dev"]),
               "jt_batch256_host_us": summary(t["jt_b_host"]), "jt_batch256_device_us": summary(t["jt_b_dev"])}
    text = json.dumps(rec)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
