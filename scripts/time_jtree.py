"""Timing of exact inference by junction-tree propagation (bn_jt_*) on one MI355X next to sum-product belief propagation, in the
same process on the same library.  A record, not a gate.

  single   tests/golden/alarm_shaped.dsc (37 nodes, 27 cliques, state in LDS), 10 % hard evidence: one bn_jt_run against one
           bn_bp_run on the one-workgroup path at --eps.  Per call the host clock around it (the call synchronises) and the device
           time: for the junction tree HIP events around the launch (option "timing", bn_get_info "jt_last_kernel_ns"), for BP the
           device clock its kernel reads itself (bn_bp_stats.sweep_devclock_ms).
  batch    256 evidence sets on the same network: bn_jt_run_batch against bn_bp_set_evidence_batch + bn_bp_run_batch_device.
  form 2   synth.grid(4, 40, 4): one bn_jt_run with the state in device scratch (the network is beyond BP's exactness anyway).
  error    the largest |BP belief - exact belief| on synth.grid(3, 3, 4) and on the ALARM-shaped network at eps 1e-9: what
           exactness buys.
After --warmup untimed rounds the two sides alternate --reps times; median, quartiles, minimum and maximum of each are reported.
One JSON object on stdout (and into --out).  Needs a GPU: there is no CPU path.

  python scripts/time_jtree.py [--reps 30] [--warmup 5] [--eps 1e-3] [--out FILE]
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
    rec = {"eps": args.eps}
    t = {k: [] for k in ("jt_host", "jt_dev", "bp_host", "bp_dev", "jtb_host", "jtb_dev", "bpb_host", "bpb_dev")}
    with Engine(alarm, device=0) as jt, Engine(alarm, device=0) as bp:
        jt.set_option("timing", 1)
        for rep in range(args.warmup + args.reps):
            a, _ = clock(lambda: jt.jt_run(ev))
            a_dev = jt.info("jt_last_kernel_ns") * 1e-3
            b, r = clock(lambda: bp.bp_run(ev, args.eps))
            assert bp.last_path() == 3, "BP did not take the one-workgroup path"
            b_dev = bp.bp_stats()["sweep_devclock_ms"] * 1e3
            c, _ = clock(lambda: jt.jt_run_batch(sets))
            c_dev = jt.info("jt_last_kernel_ns") * 1e-3
            bp.bp_set_evidence_batch(sets)
            d, _ = clock(lambda: bp.bp_run_batch_device(args.eps))
            d_dev = bp.bp_stats()["sweep_devclock_ms"] * 1e3
            if rep >= args.warmup:
                for k, x in zip(t, (a, a_dev, b, b_dev, c, c_dev, d, d_dev)):
                    t[k].append(x)
        rec["alarm"] = {"cliques": jt.info("jt_cliques"), "levels": jt.info("jt_levels"), "state_cells": jt.info("jt_state_cells"),
                        "form": jt.info("jt_last_form"), "bp_sweeps": r["sweeps"],
                        "jt_run_host_us": summary(t["jt_host"]), "jt_run_device_us": summary(t["jt_dev"]),
                        "bp_run_host_us": summary(t["bp_host"]), "bp_run_devclock_us": summary(t["bp_dev"]),
                        "jt_batch256_host_us": summary(t["jtb_host"]), "jt_batch256_device_us": summary(t["jtb_dev"]),
                        "bp_batch256_host_us": summary(t["bpb_host"]), "bp_batch256_devclock_us": summary(t["bpb_dev"])}
    big = synth.grid(4, 40, 4, seed=1)
    evb = synth.random_evidence(big, 0.1, seed=3)
    host, dev = [], []
    with Engine(big, device=0) as e:
        e.set_option("timing", 1)
        for rep in range(args.warmup + args.reps):
            a, _ = clock(lambda: e.jt_run(evb))
            if rep >= args.warmup:
                host.append(a)
                dev.append(e.info("jt_last_kernel_ns") * 1e-3)
        rec["grid4x40"] = {"cliques": e.info("jt_cliques"), "levels": e.info("jt_levels"), "state_cells": e.info("jt_state_cells"),
                           "form": e.info("jt_last_form"), "jt_run_host_us": summary(host), "jt_run_device_us": summary(dev)}
    err = {}
    for name, m in (("grid3x3", synth.grid(3, 3, 4, seed=1)), ("alarm", alarm)):
        with Engine(m, device=0) as e:
            worst = 0.0
            for seed in range(8):
                q = synth.random_evidence(m, 0.2, seed=seed) if seed else None
                exact = e.jt_run(q)["beliefs"]
                if not np.isfinite(exact).all():
                    continue
                free = np.ones(exact.size, dtype=bool)   # evidence nodes: BP reports e^2 / sum(e^2), not a posterior
                if q is not None:
                    for v in q.node[:q.ne]:
                        free[m.node_off[v]:m.node_off[v + 1]] = False
                worst = max(worst, float(np.abs(e.bp_run(q, 1e-9, 2000)["beliefs"] - exact)[free].max()))
            err[name] = worst
    rec["largest_bp_error"] = err
    text = json.dumps(rec)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
