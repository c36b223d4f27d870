"""Timing of Gibbs sampling (bn_gibbs_run) on one MI355X, with likelihood weighting on the same network for context.  A record,
not a gate.

  gibbs    tests/golden/alarm_shaped.dsc (37 nodes), 10 % hard evidence: --chains chains x --sweeps sweeps per call, the chains
           started by the caller (init_states: the states of one untimed call), so a call is the sweeps and nothing else.  Per
           call the host clock around it (the call synchronises) and the device time: HIP events around the launches (option
           "timing", bn_get_info "gibbs_last_kernel_ns").  Reported: device time per sweep, and node updates per second = chains x
           sweeps x free nodes / device time.
  lw       bn_lw_run of --lw-samples samples on the same network and evidence, host clock (the call synchronises): samples per
           second, and node draws per second = samples/s x n.  Context, not a bar: a Gibbs update reads the tables of a node's
           children, which a forward draw does not.
After --warmup untimed rounds the two alternate --reps times; median, quartiles, minimum and maximum of each are reported.
One JSON object on stdout (and into --out).  Needs a GPU: there is no CPU path.

  python scripts/time_gibbs.py [--reps 20] [--warmup 3] [--chains 4096] [--sweeps 200] [--lw-samples 4194304] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--lw-samples", type=int, default=1 << 22)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from bayesiannetwork_amd import synth
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.engine import Engine

    alarm = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    ev = synth.random_evidence(alarm, 0.1, seed=7)
    ev_state = np.full(alarm.n, -1, dtype=np.int32)
    for j in range(ev.ne):
        ev_state[int(ev.node[j])] = int(np.argmax(ev.val[ev.off[j]:ev.off[j + 1]]))
    free = int(np.count_nonzero(ev_state < 0))
    g_host, g_dev, l_host = [], [], []
    with Engine(alarm, device=0) as e:
        e.set_option("timing", 1)
        plan = e.gibbs_plan()
        start = e.gibbs_run(ev_state, args.chains, 0, seed=1)["states"]
        for rep in range(args.warmup + args.reps):
            a, r = clock(lambda: e.gibbs_run(ev_state, args.chains, args.sweeps, seed=1, init_states=start))
            a_dev = e.info("gibbs_last_kernel_ns") * 1e-3
            launches = e.info("gibbs_last_launches")
            b, _ = clock(lambda: e.lw_run(ev_state, args.lw_samples, seed=1))
            if rep >= args.warmup:
                g_host.append(a)
                g_dev.append(a_dev)
                l_host.append(b)
    dev, lw = summary(g_dev), summary(l_host)
    updates = float(args.chains) * args.sweeps * free
    rec = {"network": "alarm_shaped", "nodes": alarm.n, "free_nodes": free, "chains": args.chains, "sweeps": args.sweeps,
           "colours": plan["colours"], "lds_bytes": plan["lds_bytes"], "sweeps_per_launch": plan["sweeps_per_launch"], "launches": launches,
           "stuck": r["stuck"],
           "gibbs_run_host_us": summary(g_host), "gibbs_run_device_us": dev,
           "device_us_per_sweep": {k: dev[k] / args.sweeps for k in ("median", "q1", "q3", "min", "max")},
           "node_updates_per_s": {"median": updates / dev["median"] * 1e6, "q1": updates / dev["q3"] * 1e6, "q3": updates / dev["q1"] * 1e6},
           "lw_samples": args.lw_samples, "lw_run_host_us": lw,
           "lw_samples_per_s": {"median": args.lw_samples / lw["median"] * 1e6, "q1": args.lw_samples / lw["q3"] * 1e6,
                                "q3": args.lw_samples / lw["q1"] * 1e6},
           "lw_node_draws_per_s": {"median": args.lw_samples * alarm.n / lw["median"] * 1e6}}
    text = json.dumps(rec)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
