"""Timing of the subset lattice (bn_learn_score_subsets) on one MI355X against the only way the library had to get the same 2^m
family terms before: bn_learn_score_groups, which counts every family from the pattern table.

Shapes: random patterns over the columns of the ALARM-shaped network (tests/golden/alarm_shaped.dsc: 37 columns, arities 2-4),
--patterns rows each (default 2e3, 2e5, 1e7), child = column 0, candidates = the m other columns of the smallest arity (m = 4, 8,
12; the top family of m = 12 is beyond 4 096 cells and runs one launch per level, the others the one-launch form).  The baseline
scores the SAME families grouped so that none is scored twice: one group per subset S of cand[:-1], base S, candidate cand[-1]
(2^(m-1) groups, 2^m families).  Where that would read more than --baseline-gb from the table, a sample of the groups is timed and
scaled (flagged "baseline_is_partial").  The two are timed in one process, alternating, --reps times, warm; the best of each is
reported: host to host, the device time of the kernels (bn_info_get "learn_*_ns"), their ratios, and the lattice kernels' bytes
(from the shapes: what they read from and write to device memory) over their device time against the better of the library's
copy / triad kernels (bench.py's hbm_stream_gbs_measured).  One JSON line per shape.

  python scripts/time_subsets.py [--patterns 2e3,2e5,1e7] [--m 4,8,12] [--reps 3] [--baseline-gb 6] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_gbs(device=0):
    from bayesiannetwork_amd import _lib
    best = 0.0
    for mode in (0, 1):
        g = ctypes.c_double(0.0)
        _lib.check(_lib.lib().bn_debug_stream(device, mode, 1 << 30, 5, ctypes.byref(g)))
        best = max(best, g.value)
    return best


def lattice_bytes(k, child, cand):
    """Device-memory bytes of the lattice kernel(s), from the shapes.  Per-level form: a family of c cells derived through a
    variable of arity kx reads kx * c cells and writes c.  One-launch form: every workgroup (at most 512) reads the top table once
    and each family is written once; the intermediate steps stay in LDS."""
    ids = sorted(cand)
    m = len(cand)
    top = int(k[child]) * int(np.prod([int(k[u]) for u in ids], dtype=np.int64))
    cells = 0
    for mask in range((1 << m) - 1):
        c = int(k[child])
        kx = None
        for u in ids:
            if (mask >> cand.index(u)) & 1:
                c *= int(k[u])
            elif kx is None:
                kx = int(k[u])
        cells += c + (kx * c if top > 4096 else 0)
    if top <= 4096:
        cells += min((1 << m) - 1, 512) * top
    return 8 * cells, top


def run_shape(table, k, P, m, reps, baseline_gb, stream):
    from bayesiannetwork_amd.learning import score_groups, score_subsets
    by_arity = sorted(range(1, len(k)), key=lambda v: (int(k[v]), v))
    child, cand = 0, by_arity[:m]
    groups = [(child, sorted(cand[j] for j in range(m - 1) if (s >> j) & 1), [cand[-1]]) for s in range(1 << (m - 1))] if m else [(child, [], [])]
    group_bytes = [P * (8 + len(g[1]) + 2) for g in groups]
    budget, timed = baseline_gb * 1e9, len(groups)
    if sum(group_bytes) > budget:
        timed = max(8, int(len(groups) * budget / sum(group_bytes)))
    step = len(groups) / timed
    sample = [groups[int(i * step)] for i in range(timed)]
    scale = len(groups) / len(sample)

    def lattice():
        t0 = time.perf_counter()
        ll = score_subsets(table, child, [], cand)
        return time.perf_counter() - t0, {n: table.info(f"learn_{n}_ns") * 1e-9 for n in ("count", "lattice", "score")}, ll

    def baseline():
        t0 = time.perf_counter()
        ll = score_groups(table, sample)
        return time.perf_counter() - t0, {n: table.info(f"learn_{n}_ns") * 1e-9 for n in ("count", "score")}, ll
    lat, base = lattice(), baseline()   # (warm: code objects, allocator)
    if timed == len(groups):   # the same families, the same bits
        want = {}
        for (c, b, u), (l0, l1) in zip(groups, base[2]):
            want[tuple(b)], want[tuple(sorted(b + u))] = l0, l1
        for mask, x in enumerate(lat[2]):
            assert want[tuple(sorted(cand[j] for j in range(m) if (mask >> j) & 1))] == x, mask
    for _ in range(reps):
        r = lattice()
        lat = r if r[0] < lat[0] else lat
        r = baseline()
        base = r if r[0] < base[0] else base
    nbytes, top = lattice_bytes(k, child, cand)
    dev_lat, dev_base = sum(lat[1].values()), sum(base[1].values()) * scale
    out = {"patterns": P, "m": m, "families": 1 << m, "top_cells": top, "form": "one launch" if top <= 4096 else "per level",
           "lattice_s": lat[0], "lattice_count_kernel_s": lat[1]["count"], "lattice_kernel_s": lat[1]["lattice"],
           "lattice_score_kernel_s": lat[1]["score"], "lattice_device_s": dev_lat,
           "baseline_groups": len(groups), "baseline_groups_timed": len(sample), "baseline_is_partial": timed < len(groups),
           "baseline_s": base[0] * scale, "baseline_count_kernel_s": base[1]["count"] * scale, "baseline_score_kernel_s": base[1]["score"] * scale,
           "baseline_device_s": dev_base, "ratio_host": base[0] * scale / lat[0], "ratio_device": dev_base / dev_lat if dev_lat > 0 else 0.0,
           "lattice_bytes": nbytes, "lattice_gbs": nbytes / lat[1]["lattice"] / 1e9 if lat[1]["lattice"] > 0 else 0.0,
           "hbm_stream_gbs_measured": stream}
    out["lattice_frac_of_stream"] = out["lattice_gbs"] / stream if stream else 0.0
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patterns", default="2e3,2e5,1e7")
    ap.add_argument("--m", default="4,8,12")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-gb", type=float, default=6.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    from bayesiannetwork_amd.dsc import load_dsc
    from bayesiannetwork_amd.evaluation import InfoTable
    k = [int(x) for x in load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0].k]
    stream = stream_gbs()
    lines = []
    for size in a.patterns.split(","):
        P = int(float(size))
        rng = np.random.default_rng(P)
        pats = np.stack([rng.integers(0, kk, P, dtype=np.uint8) for kk in k], axis=1)
        counts = rng.integers(1, 1000, P).astype(np.uint64)
        with InfoTable(pats, counts, k, device=0) as table:
            del pats
            for m in (int(x) for x in a.m.split(",")):
                lines.append(run_shape(table, k, P, m, a.reps, a.baseline_gb, stream))
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
