"""Timing of the tree learners (bn_learn_tree) on one MI355X: the conditional all-pairs kernel beside the unconditional
one, beside the same matrix from single bn_info_entropy calls, the spanning-tree kernel, and the learners host to host.

Tables: `alarm` -- --draws forward samples of the ALARM-shaped network (tests/golden/alarm_shaped.dsc: 37 nodes), the class the first
column of arity 4; `dag_1024` -- the 1 024-column, 2^18-sample table of scripts/time_entropy.py (every arity 4), the class column 0.

Reported, not asserted, one JSON line per table and one for the spanning tree; each figure as median and range over --reps warm
repetitions:
  (a) cond_ms: device time of the conditional kernel; pairs_ms: of the unconditional kernel over the same features; k_class;
      ratio = cond_ms / (k_class * pairs_ms): what the mask costs per pass over the table;
  (b) single_calls_s: the same matrix as C(m, 2) + m bn_info_entropy({x, y, class}) calls, TIMED ON --sample PAIRS AND SCALED;
  (c) tree_us and tree_us_per_step at m = 37, 1 024, 4 096: the spanning-tree kernel inside bn_learn_tree (bn_info_get "tree_ns") on a
      table of m random binary columns, and bn_tree_max_spanning host to host on that call's matrix;
  (d) chow_liu_s, tan_s: the learners host to host, and tree_us: the spanning-tree kernel inside them.

  python scripts/time_tree.py [--tables alarm,dag_1024] [--draws 2000] [--reps 5] [--sample 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def alarm_table(draws):
    import learning_refs as LR
    from bayesiannetwork_amd.dsc import load_dsc
    model, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    table = LR.sample_table(model, draws, 21)
    return table.pats, table.counts, model.k


def time_table(name, pats, counts, k, reps, sample):
    import numpy as np
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import TAN, ChowLiu
    cls = int(np.flatnonzero(np.asarray(k) == 4)[0])
    feats = [v for v in range(len(k)) if v != cls]
    m = len(feats)
    out = {"table": name, "columns": len(k), "patterns": int(len(counts)), "samples": int(np.asarray(counts).sum()), "class": cls,
           "k_class": int(k[cls]), "features": m, "reps": reps}
    with InfoTable(pats, counts, k, device=0) as t:
        out["digit_passes"] = t.info("digit_passes")
        t.pair_entropies(feats)                       # (the first call of a process also loads the code objects)
        t.cond_pair_entropies(cls, feats)
        pairs_ms, cond_ms = [], []
        for _ in range(reps):                         # the two alternate in one process
            t.pair_entropies(feats)
            pairs_ms.append(t.last_pairs_ms())
            t.cond_pair_entropies(cls, feats)
            cond_ms.append(t.info("cond_pairs_ns") * 1e-6)
        out["pairs_ms"], out["cond_ms"] = spread(pairs_ms), spread(cond_ms)
        out["ratio_per_pass"] = out["cond_ms"]["median"] / (out["k_class"] * out["pairs_ms"]["median"])
        rng = np.random.default_rng(3)
        chosen = [tuple(int(v) for v in rng.choice(feats, 2, replace=False)) for _ in range(sample)]
        t.entropy([chosen[0][0], chosen[0][1], cls])
        singles = []
        for _ in range(reps):
            h0 = time.perf_counter()
            for x, y in chosen:
                t.entropy([x, y, cls])
            singles.append((time.perf_counter() - h0) / sample * (m * (m - 1) // 2 + m))
        out["single_calls_s"] = dict(spread(singles), sampled_pairs=sample, scaled_to=m * (m - 1) // 2 + m)
        ChowLiu()(t)
        TAN(cls)(t)
        cl_s, tan_s, cl_tree, tan_tree = [], [], [], []
        for _ in range(reps):
            h0 = time.perf_counter()
            ChowLiu()(t, feats)
            cl_s.append(time.perf_counter() - h0)
            cl_tree.append(t.info("tree_ns") * 1e-3)
            h0 = time.perf_counter()
            TAN(cls)(t)
            tan_s.append(time.perf_counter() - h0)
            tan_tree.append(t.info("tree_ns") * 1e-3)
        out["chow_liu_s"], out["tan_s"] = spread(cl_s), spread(tan_s)
        out["chow_liu_tree_us"], out["tan_tree_us"] = spread(cl_tree), spread(tan_tree)
    return out


def time_spanning(reps):
    import numpy as np
    from bayesiannetwork_amd.evaluation import InfoTable
    from bayesiannetwork_amd.learning import ChowLiu, max_spanning_tree
    out = {"spanning_tree": [], "reps": reps}
    for m in (37, 1024, 4096):
        pats = np.random.default_rng(m).integers(0, 2, (512, m)).astype(np.uint8)
        with InfoTable(pats, np.ones(512, np.uint64), np.full(m, 2, np.int32), device=0) as t:
            w = ChowLiu()(t).matrix
            max_spanning_tree(w, 0, device=0)
            us, learn, host = [], [], []
            for _ in range(reps):
                h0 = time.perf_counter()
                ChowLiu()(t)
                learn.append(time.perf_counter() - h0)
                us.append(t.info("tree_ns") * 1e-3)
                h0 = time.perf_counter()
                max_spanning_tree(w, 0, device=0)
                host.append(time.perf_counter() - h0)
        out["spanning_tree"].append({"m": m, "tree_us": spread(us), "tree_us_per_step": spread([u / (m - 1) for u in us]),
                                     "chow_liu_s": spread(learn), "max_spanning_tree_host_s": spread(host)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default="alarm,dag_1024")
    ap.add_argument("--draws", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []
    for name in [s for s in args.tables.split(",") if s]:
        if name == "alarm":
            pats, counts, k = alarm_table(args.draws)
        elif name == "dag_1024":
            import time_entropy
            pats, counts, k = time_entropy.shape_dag()
        else:
            raise SystemExit(f"unknown table {name}")
        lines.append(json.dumps(time_table(name, pats, counts, k, args.reps, args.sample)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(time_spanning(args.reps)))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
