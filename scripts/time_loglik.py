"""Timing of the log-likelihood scores (bn_score_rows, bn_score_nodes) on one MI355X.

Shapes:
  alarm_1e6 / alarm_1e7: the ALARM-shaped network (tests/golden/alarm_shaped.dsc, 37 nodes) with 10^6 / 10^7 patterns
  dag10k_1e5:            BASELINE configs[1] (10 000-node random DAG, k = 4, <= 4 parents) with 10^5 patterns
  mixed10k_1e5:          bench.py's `mixed10k` (10 000 nodes, arities 2-5, <= 3 parents) with 10^5 patterns
The patterns are uniform random states of count 1 (at these sizes practically all distinct; what a pattern scores does not
change what the kernels do).  Per shape: device-event times of the row kernel(s) and of the node pass (family counts +
node sums; the counting kernel also with one workgroup per node, option "score_splits" = 1), best of --reps; patterns/s;
achieved bytes/s of the row kernel over the measured stream rate -- bytes = (1 + parents) state bytes per node and pattern
summed over the nodes, plus 8 P of output, from the shapes alone (the gathers from the log table are not counted: it stays
in cache) -- against the better of the library's copy / triad kernels (bn_debug_stream, bench.py's
hbm_stream_gbs_measured); and the time of the numpy restatement of the row sums on up to 16 threads for the same input
(measured on at most --numpy-patterns patterns and scaled).  Prints one JSON line per shape; --out writes them to a file.

  python scripts/time_loglik.py [--shapes alarm_1e6,alarm_1e7,dag10k_1e5,mixed10k_1e5] [--reps 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def network(name):
    from bayesiannetwork_amd import synth
    from bayesiannetwork_amd.dsc import load_dsc
    if name == "alarm":
        return load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    if name == "dag10k":
        return synth.random_dag(10000, 4, 64, 4, seed=1)
    return synth.random_dag(10000, 3, 16, [2, 3, 4, 3, 2, 4, 5], seed=20)


def random_patterns(k, P, seed):
    r = np.random.default_rng(seed)
    pats = np.empty((P, len(k)), np.uint8)
    for v, kv in enumerate(k):
        pats[:, v] = r.integers(0, kv, P, dtype=np.uint8)
    return pats


def numpy_rows(model, L, pats):
    """the row sums in the header's order (segments of 256 node ids), one chunk of patterns"""
    total = np.zeros(pats.shape[0])
    for v0 in range(0, model.n, 256):
        acc = np.zeros(pats.shape[0])
        for v in range(v0, min(model.n, v0 + 256)):
            row = np.zeros(pats.shape[0], np.int64)
            for u in model.parents(v):
                row = row * int(model.k[u]) + pats[:, u]
            acc = acc + L[int(model.cpt_off[v]) + row * int(model.k[v]) + pats[:, v]]
        total = total + acc
    return total


def stream_gbs(device=0):
    from bayesiannetwork_amd import _lib
    best = 0.0
    for mode in (0, 1):
        g = ctypes.c_double(0.0)
        _lib.check(_lib.lib().bn_debug_stream(device, mode, 1 << 30, 5, ctypes.byref(g)))
        best = max(best, g.value)
    return best


def run_shape(name, reps, numpy_patterns, stream):
    from bayesiannetwork_amd.engine import Engine
    from bayesiannetwork_amd.evaluation import InfoTable, log_cpt, log_likelihood_nodes, log_likelihood_rows
    net, size = name.rsplit("_", 1)
    P = int(float(size))
    model = network(net)
    pats = random_patterns(model.k, P, seed=5)
    parents = int(model.in_ptr[-1])
    row_bytes = (model.n + parents) * P + 8 * P
    out = {"shape": name, "nodes": model.n, "edges": parents, "cpt_entries": int(model.cpt_off[-1]), "patterns": P,
           "row_kernel_bytes": row_bytes, "hbm_stream_gbs_measured": stream}
    t0 = time.perf_counter()
    with Engine(model, device=0) as eng, InfoTable(pats, np.ones(P, np.uint64), model.k, device=0) as table:
        out["upload_ms"] = (time.perf_counter() - t0) * 1e3
        rows_ms, count_ms, nodes_ms, count1_ms, h2h_rows, h2h_nodes = [], [], [], [], [], []
        for _ in range(reps + 1):   # (the first call also makes the log table and loads the code objects: dropped)
            t0 = time.perf_counter()
            ll = log_likelihood_rows(eng, table)
            h2h_rows.append((time.perf_counter() - t0) * 1e3)
            rows_ms.append(eng.info("score_rows_ns") * 1e-6)
            t0 = time.perf_counter()
            log_likelihood_nodes(eng, table)
            h2h_nodes.append((time.perf_counter() - t0) * 1e3)
            count_ms.append(eng.info("score_count_ns") * 1e-6)
            nodes_ms.append(eng.info("score_nodes_ns") * 1e-6)
        eng.set_option("score_splits", 1)
        for _ in range(reps):
            log_likelihood_nodes(eng, table)
            count1_ms.append(eng.info("score_count_ns") * 1e-6)
        L = log_cpt(eng)
    rk = min(rows_ms[1:])
    out.update({"rows_kernel_ms": rk, "rows_patterns_per_s": P / (rk * 1e-3), "rows_gbs": row_bytes / (rk * 1e-3) / 1e9,
                "rows_frac_of_stream": row_bytes / (rk * 1e-3) / 1e9 / stream, "rows_host_to_host_ms": min(h2h_rows[1:]),
                "count_kernel_ms": min(count_ms[1:]), "count_kernel_one_workgroup_per_node_ms": min(count1_ms),
                "node_sum_kernel_ms": min(nodes_ms[1:]), "nodes_patterns_per_s": P / ((min(count_ms[1:]) + min(nodes_ms[1:])) * 1e-3),
                "nodes_host_to_host_ms": min(h2h_nodes[1:])})
    # the numpy restatement on up to 16 threads, chunks of patterns
    Pn = min(P, numpy_patterns)
    threads = min(16, os.cpu_count() or 1)
    chunks = np.array_split(np.arange(Pn), threads)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda idx: numpy_rows(model, L, pats[idx[0]:idx[-1] + 1]), [c for c in chunks if len(c)]))
    dt = time.perf_counter() - t0
    ref = np.concatenate(parts)
    out.update({"numpy_threads": threads, "numpy_patterns_timed": Pn, "numpy_ms_scaled_to_all_patterns": dt * 1e3 * P / Pn,
                "numpy_patterns_per_s": Pn / dt, "rows_equal_numpy_bits": bool(np.array_equal(ref.view(np.uint64), ll[:Pn].view(np.uint64)))})
    out["rows_speedup_over_numpy"] = out["numpy_ms_scaled_to_all_patterns"] / rk
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="alarm_1e6,alarm_1e7,dag10k_1e5,mixed10k_1e5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-patterns", type=int, default=1000000)
    ap.add_argument("--out")
    a = ap.parse_args()
    stream = stream_gbs()
    lines = []
    for name in a.shapes.split(","):
        r = run_shape(name, a.reps, a.numpy_patterns, stream)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
