"""Timing of bn_info_pair_entropies (all-pairs joint entropies, int8 matrix cores) on one MI355X.

Shapes:
  onehot_2048: n = 2048 columns of arity 4, P = 2^20 random patterns of count 1 (K = 8192 slot columns;
               P * K^2 = 7.0e13 int ops for the upper triangle with its diagonal blocks)
  dag_1024:    the pattern table of BASELINE configs[1] (10 k-node random DAG, k = 4) sampled the way
               LikelihoodWeighting.make_samples samples one unit (no evidence, 2^18 samples), over 1 024 of its nodes
Per shape: the table upload (bn_info_create: copy, device transpose, state check), the host-to-host
time of pair_entropies, the device time of its all-pairs kernel (events), achieved int8 ops/s over the
spec-derived peak (5.0e15: 2x the 2.5 PF dense bf16 figure, MI355X_MICROARCH), and a torch yardstick:
a bf16 one-hot X^T X chunked over the patterns so that its fp32 sums stay exact (< 2^24), plus the
entropy epilogue in torch.  Prints one JSON line per shape; --out writes them to a file.

  python scripts/time_entropy.py [--shapes onehot_2048,dag_1024] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

I8_PEAK = 5.0e15


def shape_onehot(seed=1):
    r = np.random.default_rng(seed)
    n, P = 2048, 1 << 20
    pats = np.empty((P, n), np.uint8)
    for i in range(0, P, 1 << 16):
        pats[i:i + (1 << 16)] = r.integers(0, 4, (min(1 << 16, P - i), n), dtype=np.uint8)
    return pats, np.ones(P, np.uint64), np.full(n, 4, np.int32)


def shape_dag(seed=1):
    from bayesiannetwork_amd import synth
    from bayesiannetwork_amd.engine import Engine
    g = synth.random_dag(10000, 4, 64, 4, seed=1)
    nodes = np.sort(np.random.default_rng(seed).choice(g.n, 1024, replace=False))
    total, piece = 1 << 18, 1 << 14
    cols = np.empty((total, len(nodes)), np.uint8)
    ev = np.full(g.n, -1, np.int32)
    with Engine(g, device=0) as eng:
        for b in range(0, total, piece):
            eng.lw_run(ev, piece, 0x5EED, b)
            states, _ = eng.lw_states(piece)
            cols[b:b + piece] = states[:, nodes]
    pats, cnt = np.unique(cols, axis=0, return_counts=True)
    return np.ascontiguousarray(pats), cnt.astype(np.uint64), g.k[nodes].astype(np.int32)


def torch_yardstick(torch, pats, counts, k, reps):
    """One-hot X [P][K] bf16 built on the device from the resident states, X^T diag(w) X by torch.mm in P-chunks
    with fp32 output (exact: every sum < 2^24), and H(x, y) of every pair in torch.  Columns of one arity only
    (both shapes here); counts <= 256 (exact in bf16)."""
    dev = torch.device("cuda:0")
    kk = int(k[0])
    assert (k == kk).all() and counts.max() <= 256 and int(counts.sum()) < (1 << 24)
    n = len(k)
    K = n * kk
    st = torch.from_numpy(pats).to(dev)
    w = torch.from_numpy(counts.astype(np.float32)).to(dev).to(torch.bfloat16)
    N = float(counts.sum())
    chunk = min(len(counts), 1 << 15)

    def run():
        acc = torch.zeros((K, K), dtype=torch.float32, device=dev)
        for b in range(0, len(counts), chunk):
            x = torch.nn.functional.one_hot(st[b:b + chunk].long(), kk).reshape(-1, K).to(torch.bfloat16)
            acc += torch.mm((x * w[b:b + chunk, None]).T, x, out_dtype=torch.float32)
        p = acc.reshape(n, kk, n, kk).permute(0, 2, 1, 3).double() / N
        t = torch.where(p > 0, p * torch.log2(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))
        return -t.sum(dim=(2, 3))

    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hxy = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return min(times) * 1e3, hxy.cpu().numpy()


def time_shape(name, reps, torch):
    from bayesiannetwork_amd.evaluation import InfoTable
    t0 = time.perf_counter()
    pats, counts, k = shape_onehot() if name == "onehot_2048" else shape_dag()
    gen_s = time.perf_counter() - t0
    slots = np.array([max(2, 1 << int(np.ceil(np.log2(max(kk, 2))))) for kk in k])
    K = int(slots.sum())
    P = len(counts)
    t0 = time.perf_counter()
    tab = InfoTable(pats, counts, k, device=0)
    upload_ms = (time.perf_counter() - t0) * 1e3
    out = tab.pair_entropies(mi=True)   # warm-up (code objects)
    h2h, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = tab.pair_entropies(mi=True)
        h2h.append((time.perf_counter() - t0) * 1e3)
        dev.append(tab.last_pairs_ms())
    single = [tab.entropy([x, y]) for x, y in ((0, 1), (5, len(k) - 1), (len(k) // 2, 3))]
    bits_ok = all(out["hxy"][x, y] == s for (x, y), s in zip(((0, 1), (5, len(k) - 1), (len(k) // 2, 3)), single))
    tab.close()
    ops = float(P) * K * K
    res = {"shape": name, "n": int(len(k)), "P": P, "K_slots": K, "int_ops_upper": ops, "digit_passes": 1,
           "table_gen_s": round(gen_s, 2), "upload_ms": round(upload_ms, 2),
           "pair_entropies_h2h_ms_min": round(min(h2h), 3), "pair_kernel_device_ms_min": round(min(dev), 3),
           "pair_kernel_device_ms_all": [round(x, 3) for x in dev],
           "achieved_int8_ops_per_s": ops / (min(dev) * 1e-3), "fraction_of_i8_peak": ops / (min(dev) * 1e-3) / I8_PEAK,
           "i8_peak_assumed": I8_PEAK, "single_call_bits_equal": bits_ok}
    if torch is not None:
        ms, hxy_t = torch_yardstick(torch, pats, counts, k, reps)
        res["torch_bf16_yardstick_ms_min"] = round(ms, 3)
        res["torch_max_abs_diff"] = float(np.abs(hxy_t - out["hxy"]).max())
        res["faster_than_torch"] = min(h2h) < ms
        res["speedup_vs_torch_h2h"] = round(ms / min(h2h), 2)
    res["goal_0.3_of_peak_met"] = res["fraction_of_i8_peak"] >= 0.3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="onehot_2048,dag_1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch = None
    if not a.no_torch:
        import torch as _t
        torch = _t
    lines = []
    for name in a.shapes.split(","):
        res = time_shape(name, a.reps, torch)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
