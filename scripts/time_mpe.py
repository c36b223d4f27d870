"""Timing of max-product belief propagation (bn_mpe_run) on one MI355X next to sum-product (bn_bp_run) on the same network, the same
evidence and the same number of sweeps, in the same process.

  one workgroup      tests/golden/alarm_shaped.dsc (37 nodes): both kernels keep the state in LDS and run the whole query in one launch
  several workgroups synth.random_dag(1000, 3, 16, [2, 3, 4, 3, 2, 4, 5], seed=14): max-product runs one launch per sweep and reads
                     its control record once per group of launches (option "mpe_group": every size in --groups is timed); sum-
                     product runs the several-workgroup kernel with its grid barrier (one launch per run)

Every run is cut at a fixed number of sweeps (eps = 0: no sweep's residual is below it), so both sides do the same work.
  device time per sweep   the device's 100 MHz clock read by the kernels themselves (bn_get_info "mpe_last_device_ns"; bn_bp_stats
                          sweep_devclock_ms) over --sweeps sweeps: first sweep's start to the run's end
  host-to-host per query  a host clock around the whole call (evidence in, results out, the call's synchronisation included) at
                          --query-sweeps sweeps
After --warmup untimed rounds the two sides alternate --reps times; median, quartiles, minimum and maximum of each are reported.
The bar of the one-workgroup form: the max-product median must not exceed the sum-product median by more than the spread
(maximum - minimum; the inter-quartile range is printed beside it) of the sum-product repetitions of this run.
One JSON object per network on stdout (and into --out).  Needs a GPU: there is no CPU path.

  python scripts/time_mpe.py [--reps 30] [--warmup 5] [--sweeps 1000] [--query-sweeps 16] [--groups 1,2,4,8,16,32,64] [--out FILE]
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
    return {"median": float(med), "q1": float(q1), "q3": float(q3), "iqr": float(q3 - q1), "min": float(a[0]), "max": float(a[-1]),
            "range": float(a[-1] - a[0]), "n": int(a.size)}


def alternate(eng, ev, sweeps, reps, warmup, host_clock):
    """max-product and sum-product in turn, `sweeps` sweeps each; returns per-repetition (mpe, bp) figures: device nanoseconds per sweep,
    or host microseconds per call with host_clock"""
    mpe, bp = [], []
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        m = eng.mpe_run(ev, 0.0, sweeps)
        t1 = time.perf_counter()
        b = eng.bp_run(ev, 0.0, sweeps)
        t2 = time.perf_counter()
        assert m["sweeps"] == sweeps and b["sweeps"] == sweeps, (m["sweeps"], b["sweeps"])
        if rep < warmup:
            continue
        if host_clock:
            mpe.append((t1 - t0) * 1e6)
            bp.append((t2 - t1) * 1e6)
        else:
            # (the clock reads of the two are taken the same way: start of the first sweep to the end of the run)
            mpe.append(eng.info("mpe_last_device_ns") / sweeps)
            bp.append(eng.bp_stats()["sweep_devclock_ms"] * 1e6 / sweeps)
    return mpe, bp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=1000)
    ap.add_argument("--query-sweeps", type=int, default=16)
    ap.add_argument("--groups", default="1,2,4,8,16,32,64")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from bayesiannetwork_amd import synth
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.engine import Engine
    records = []

    # ---- one workgroup
    alarm = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    ev = synth.random_evidence(alarm, 0.1, seed=7)
    with Engine(alarm, device=0) as eng:
        assert eng.info("mpe_form") == 1
        dev_m, dev_b = alternate(eng, ev, args.sweeps, args.reps, args.warmup, False)
        assert eng.info("mpe_last_form") == 1 and eng.last_path() == 3, "sum-product did not take the one-workgroup path"
        host_m, host_b = alternate(eng, ev, args.query_sweeps, args.reps, args.warmup, True)
    sm, sb = summary(dev_m), summary(dev_b)
    records.append({"network": "alarm_shaped", "form": 1, "sweeps": args.sweeps, "query_sweeps": args.query_sweeps,
                    "device_ns_per_sweep": {"max_product": sm, "sum_product": sb},
                    "host_us_per_query": {"max_product": summary(host_m), "sum_product": summary(host_b)},
                    "bar": {"excess_ns": sm["median"] - sb["median"], "sum_product_range_ns": sb["range"], "sum_product_iqr_ns": sb["iqr"],
                            "within_range": sm["median"] - sb["median"] <= sb["range"], "within_iqr": sm["median"] - sb["median"] <= sb["iqr"]}})

    # ---- several workgroups: every group size
    big = synth.random_dag(1000, 3, 16, [2, 3, 4, 3, 2, 4, 5], seed=14)
    evb = synth.random_evidence(big, 0.1, seed=7)
    sweeps = min(args.sweeps, 256)   # (one launch per sweep: a few hundred launches are a long enough window)
    with Engine(big, device=0) as eng:
        assert eng.info("mpe_form") == 2
        rec = {"network": "random_dag(1000, 3, 16, [2,3,4,3,2,4,5], seed=14)", "form": 2, "parts": eng.info("mpe_parts"), "sweeps": sweeps,
               "query_sweeps": args.query_sweeps, "groups": {}}
        for g in [int(x) for x in args.groups.split(",")]:
            eng.set_option("mpe_group", g)
            dev_m, dev_b = alternate(eng, evb, sweeps, max(5, args.reps // 3), 2, False)
            host_m, host_b = alternate(eng, evb, args.query_sweeps, max(5, args.reps // 3), 2, True)
            rec["groups"][str(g)] = {"device_ns_per_sweep": {"max_product": summary(dev_m), "sum_product": summary(dev_b)},
                                     "host_us_per_query": {"max_product": summary(host_m), "sum_product": summary(host_b)}}
        rec["sum_product_path"] = eng.last_path()
    records.append(rec)

    text = "\n".join(json.dumps(r) for r in records)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
