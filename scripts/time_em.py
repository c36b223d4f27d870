"""Timing of the expectation-maximisation E-step and M-step (bn_em_*) on one MI355X next to the batched sum-product run
(bn_bp_run_batch_device) over the same rows as evidence sets, in the same process on the same library.

  network   tests/golden/alarm_shaped.dsc (37 nodes): one workgroup per row, state in LDS
  table     --rows distinct forward samples of the network (default 4 096) with --missing of the cells blanked (default 25 %), count 1
  E-step    bn_get_info "em_estep_ns": device events around the E-step's kernels (one em_small_kernel launch per chunk of rows and
            the accumulating kernel behind it); per pattern = that over the rows
            The same E-step with every run cut after ONE sweep is timed beside it: what is left is the kernel's set-up and epilogue
            (tables and evidence into LDS, the family pass, chunk x entries doubles written) and the accumulating kernel.
  M-step    bn_get_info "em_mstep_ns" of a one-iteration bn_em_fit
  BP batch  the rows as hard evidence, 256 sets per bn_bp_set_evidence_batch, a host clock around each bn_bp_run_batch_device (the call
            synchronises), summed over the table: the cost of the inference alone, launches and host waits included.  The host clock
            around the whole bn_em_expected_counts call (table upload included) is printed beside it.
Both sides use the same eps and the same sweep cap.  After --warmup untimed rounds the two sides alternate --reps times; median,
quartiles, minimum and maximum of each are reported, and the ratio of the medians.  One JSON object on stdout (and into --out).
Needs a GPU: there is no CPU path.

  python scripts/time_em.py [--rows 4096] [--missing 0.25] [--reps 20] [--warmup 3] [--eps 1e-3] [--cap 100] [--out FILE]
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


def forward_samples(model, count, rng):
    """`count` joint samples [count][n] uint8, nodes drawn parents first."""
    n = model.n
    parents = [[int(u) for u in model.parents(v)] for v in range(n)]
    order, placed = [], set()
    while len(order) < n:
        for v in range(n):
            if v not in placed and all(u in placed for u in parents[v]):
                order.append(v)
                placed.add(v)
    x = np.zeros((count, n), dtype=np.int64)
    for v in order:
        row = np.zeros(count, dtype=np.int64)
        for u in parents[v]:
            row = row * int(model.k[u]) + x[:, u]
        cdf = np.cumsum(model.cpt_of(v)[row], axis=1)
        u01 = rng.random(count) * cdf[:, -1]
        x[:, v] = np.minimum((u01[:, None] >= cdf).sum(axis=1), int(model.k[v]) - 1)
    return x.astype(np.uint8)


def distinct_rows(model, rows, missing, seed):
    from bayesiannetwork_amd import MISSING
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < rows:
        block = forward_samples(model, rows, rng)
        block[rng.random(block.shape) < missing] = MISSING
        for r in block:
            key = r.tobytes()
            if key not in seen and len(out) < rows:
                seen.add(key)
                out.append(r)
    return np.ascontiguousarray(np.stack(out), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--missing", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from bayesiannetwork_amd import MISSING, Evidence
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.engine import Engine

    model = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    pats = distinct_rows(model, args.rows, args.missing, seed=17)
    counts = np.ones(args.rows, dtype=np.uint64)
    sets = [Evidence.from_dict(model, {int(v): int(r[v]) for v in range(model.n) if int(r[v]) != MISSING}) for r in pats]
    batches = [sets[b:b + 256] for b in range(0, len(sets), 256)]
    S = int(model.cpt_off[-1])
    estep, estep_host, mstep, fit_estep, bp_host, estep_one = [], [], [], [], [], []
    with Engine(model, device=0) as eng:
        assert eng.info("em_eligible") == 1
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            E, sweeps = eng.em_expected_counts(pats, counts, args.eps, args.cap)
            t1 = time.perf_counter()
            e_ns = eng.info("em_estep_ns")
            eng.em_expected_counts(pats, counts, args.eps, 1)   # every run cut after ONE sweep: set-up, epilogue and the sums remain
            one_ns = eng.info("em_estep_ns")
            eng.em_fit(pats, counts, max_iters=1, tol=0.0, bp_eps=args.eps, bp_max_sweeps=args.cap)
            f_ns, m_ns = eng.info("em_estep_ns"), eng.info("em_mstep_ns")
            bp_s, bp_sweeps = 0.0, []
            for b in batches:
                eng.bp_set_evidence_batch(b)
                t2 = time.perf_counter()
                r = eng.bp_run_batch_device(args.eps, args.cap)
                bp_s += time.perf_counter() - t2
                bp_sweeps.append(r["sweeps"])
            assert eng.last_path() == 3, "the batch did not take the one-workgroup path"
            assert np.array_equal(np.concatenate(bp_sweeps), sweeps), "the two sides did not run the same sweeps"
            if rep < args.warmup:
                continue
            estep.append(e_ns * 1e-3)
            estep_one.append(one_ns * 1e-3)
            estep_host.append((t1 - t0) * 1e6)
            fit_estep.append(f_ns * 1e-3)
            mstep.append(m_ns * 1e-3)
            bp_host.append(bp_s * 1e6)
        capped, skipped = eng.info("em_capped"), eng.info("em_skipped")
    se, sb = summary(estep), summary(bp_host)
    rec = {"network": "alarm_shaped", "rows": args.rows, "missing": args.missing, "entries": S, "eps": args.eps, "cap": args.cap,
           "sweeps_total": int(sweeps.sum()), "sweeps_max": int(sweeps.max()), "capped": capped, "skipped_families": skipped,
           "estep_device_us": se, "estep_device_ns_per_pattern": se["median"] * 1e3 / args.rows,
           "estep_one_sweep_device_us": summary(estep_one), "estep_call_host_us": summary(estep_host), "fit_estep_device_us": summary(fit_estep), "mstep_device_us": summary(mstep),
           "bp_batch_host_us": sb, "bp_batch_ns_per_pattern": sb["median"] * 1e3 / args.rows, "bp_batch_calls": len(batches),
           "estep_over_bp_batch": se["median"] / sb["median"],
           "b_bytes_written_and_read": 2 * 8 * S * args.rows}
    text = json.dumps(rec)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
