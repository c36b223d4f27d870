"""Timing of structure learning (bn_learn_*, bayesiannetwork_amd.learning) on one MI355X against the only way the library had
to do the same thing before: the loop over the public API -- per candidate edge fit_cpt of the whole graph, an Engine, AIC / MDL.

Shapes:
  alarm_1e5 / alarm_1e6: the ALARM-shaped network (tests/golden/alarm_shaped.dsc, 37 nodes), 10^5 / 10^6 forward samples; full
                         greedy from the empty graph, AIC and MDL; the public-API loop in full (all 666 decisions)
  dag1000_1e5:           synth.random_dag(1000, 3, 16, [2, 3, 4], seed=11), 10^5 forward samples; full greedy, MDL; the public-API
                         loop on the FIRST --loop-decisions decisions only (default 200), scaled to all decisions beside the figure
Equal samples are merged (the table holds distinct patterns with counts).  Child order and tails: default_rng(1) / default_rng(2 + i).
The two are timed in the same call, alternating, --reps times; the best of each is reported: seconds per learned structure
(host to host), their ratio, passes and families scored, the device time of the two kernels, and for the counting kernel the bytes
it has to read -- per chunk of G candidates P * (8 + |base| + 1 + G), from the shapes (bn_learn_get "count_bytes") -- over its device
time, against the better of the library's copy / triad kernels (bench.py's hbm_stream_gbs_measured).  One JSON line per run.

  python scripts/time_learning.py [--shapes alarm_1e5,alarm_1e6,dag1000_1e5] [--reps 2] [--loop-decisions 200] [--out FILE]
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


def network(name):
    from bayesiannetwork_amd import synth
    from bayesiannetwork_amd.dsc import load_dsc
    if name == "alarm":
        return load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))[0]
    return synth.random_dag(1000, 3, 16, [2, 3, 4], seed=11)


def forward_samples(model, draws, seed):
    """`draws` ancestral samples, vectorised over the draws; nodes in a topological order."""
    rng = np.random.default_rng(seed)
    left = [set(model.parents(v).tolist()) for v in range(model.n)]
    order, done = [], set()
    while len(order) < model.n:
        free = [v for v in range(model.n) if v not in done and left[v] <= done]
        order += free
        done.update(free)
    x = np.zeros((draws, model.n), np.uint8)
    for v in order:
        row = np.zeros(draws, np.int64)
        for u in model.parents(v):
            row = row * int(model.k[u]) + x[:, u]
        cum = np.cumsum(model.cpt_of(v), axis=1)[row]
        x[:, v] = np.minimum((rng.random(draws)[:, None] * cum[:, -1:] > cum).sum(axis=1), int(model.k[v]) - 1)
    pats, counts = np.unique(x, axis=0, return_counts=True)
    return np.ascontiguousarray(pats), counts.astype(np.uint64)


def orders_of(n):
    children = [int(v) for v in np.random.default_rng(1).permutation(n)]
    tails = []
    for i in range(n):
        tail = children[i + 1:]
        tails.append([tail[j] for j in np.random.default_rng(2 + i).permutation(len(tail))])
    return children, tails


def stream_gbs(device=0):
    from bayesiannetwork_amd import _lib
    best = 0.0
    for mode in (0, 1):
        g = ctypes.c_double(0.0)
        _lib.check(_lib.lib().bn_debug_stream(device, mode, 1 << 30, 5, ctypes.byref(g)))
        best = max(best, g.value)
    return best


def reaches(parents, a):
    children = [[] for _ in parents]
    for v, ps in enumerate(parents):
        for u in ps:
            children[u].append(v)
    seen, stack = {a}, [a]
    while stack:
        for c in children[stack.pop()]:
            if c not in seen:
                seen.add(c)
                stack.append(c)
    return seen


def public_api_loop(model, table, pats, counts, criterion, orders, max_parents, limit):
    """The reference's greedy written on the parent library's API; stops after `limit` decisions.  Returns (seconds, decisions, edges)."""
    from bayesiannetwork_amd.engine import Engine, fit_cpt
    from bayesiannetwork_amd.evaluation import AIC, MDL
    from bayesiannetwork_amd.learning import _csr, structure_model
    ev = (AIC if criterion == "aic" else MDL)(table)

    def evaluate(parents):
        m = structure_model(model.k, *_csr(parents))
        m.cpt[:] = fit_cpt(m, pats, counts, device=0)
        with Engine(m, device=0) as eng:
            return ev(eng)
    t0 = time.perf_counter()
    parents = [[] for _ in range(model.n)]
    now, decisions, edges = evaluate(parents), 0, 0
    for child, tail in zip(*orders):
        for u in tail:
            if decisions >= limit:
                return time.perf_counter() - t0, decisions, edges
            if u in parents[child] or u in reaches(parents, child) or len(parents[child]) >= max_parents:
                continue
            nxt = [list(p) for p in parents]
            nxt[child] = sorted(nxt[child] + [u])
            score = evaluate(nxt)
            decisions += 1
            if score < now:
                parents, now, edges = nxt, score, edges + 1
    return time.perf_counter() - t0, decisions, edges


def learner_run(table, criterion, orders, max_parents):
    from bayesiannetwork_amd.learning import Learner
    t0 = time.perf_counter()
    with Learner(table, None, criterion, max_parents) as L:
        for child, tail in zip(*orders):
            L.try_parents(child, tail)
        dt = time.perf_counter() - t0
        info = {name: L.info(name) for name in ("families_scored", "passes", "count_ns", "score_ns", "count_bytes", "edges")}
        return dt, info, L.score()


def run_shape(name, reps, loop_decisions, stream):
    from bayesiannetwork_amd.evaluation import InfoTable
    net, size = name.rsplit("_", 1)
    draws = int(float(size))
    model = network(net)
    pats, counts = forward_samples(model, draws, seed=5)
    orders = orders_of(model.n)
    max_parents = 6 if net == "alarm" else 4
    total_decisions = model.n * (model.n - 1) // 2
    lines = []
    with InfoTable(pats, counts, model.k, device=0) as table:
        for criterion in (("aic", "mdl") if net == "alarm" else ("mdl",)):
            limit = total_decisions if net == "alarm" else loop_decisions
            learner_run(table, criterion, orders, max_parents)   # (warm: code objects, allocator)
            best, best_loop = None, None
            for _ in range(reps):
                r = learner_run(table, criterion, orders, max_parents)
                best = r if best is None or r[0] < best[0] else best
                lp = public_api_loop(model, table, pats, counts, criterion, orders, max_parents, limit)
                best_loop = lp if best_loop is None or lp[0] < best_loop[0] else best_loop
            dt, info, score = best
            loop_s, loop_dec, loop_edges = best_loop
            loop_full = loop_s * total_decisions / max(loop_dec, 1)
            count_s = info["count_ns"] * 1e-9
            out = {"shape": name, "criterion": criterion, "nodes": model.n, "draws": draws, "patterns": int(len(counts)),
                   "max_parents": max_parents, "learner_s": dt, "learner_edges": info["edges"], "learner_score": score,
                   "passes": info["passes"], "families_scored": info["families_scored"],
                   "count_kernel_s": count_s, "score_kernel_s": info["score_ns"] * 1e-9, "count_bytes": info["count_bytes"],
                   "count_gbs": info["count_bytes"] / count_s / 1e9 if count_s > 0 else 0.0, "hbm_stream_gbs_measured": stream,
                   "public_loop_decisions_timed": loop_dec, "public_loop_s_timed": loop_s, "public_loop_edges_in_those": loop_edges,
                   "public_loop_is_partial": loop_dec < total_decisions, "public_loop_s_scaled_to_all_decisions": loop_full,
                   "ratio_loop_over_learner": loop_full / dt}
            out["count_frac_of_stream"] = out["count_gbs"] / stream if stream else 0.0
            print(json.dumps(out), flush=True)
            lines.append(out)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="alarm_1e5,alarm_1e6,dag1000_1e5")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--loop-decisions", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    stream = stream_gbs()
    lines = []
    for name in a.shapes.split(","):
        lines += run_shape(name, a.reps, a.loop_decisions, stream)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
