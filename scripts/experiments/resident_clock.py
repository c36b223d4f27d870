# Phase stamps of one iteration (the sixth) of the resident kernel and of the run's fixed cost (kernel entry, CPT image,
# first sweep, last verdict, finalize), every wave: needs the diagnostic library
#   (cd build/dbg_csrc && make EXTRA=-DBN_TILE_CLOCK OUT=../libbn_dbg.so)   and   BN_MI355X_LIB=build/libbn_dbg.so
# Grid-barrier form (second argument 0): every phase again by half of the block -- waves 0-3 and their SIMD partners 4-7 -- with the
# gap between the halves at "sweep issued" (EXPERIMENTS R21; EXTRA="-DBN_TILE_CLOCK -DBN_RES_PRIO=n" stamps another priority schedule),
# and the collecting wave of every block: poll returned -> verdict written -> block released (EXPERIMENTS R22)
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bayesiannetwork_amd import _lib, synth  # noqa: E402
from bayesiannetwork_amd.engine import Engine  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 316
flow = int(sys.argv[2]) if len(sys.argv) > 2 else 1  # 1: dataflow form (a wave waits for its neighbour tiles), 0: grid barrier
g = synth.grid(rows, rows, 4, seed=2)
ev = synth.random_evidence(g, 0.01, seed=7)
L = _lib.lib()
with Engine(g) as e:
    e.set_option("multisweep", 2)
    e.set_option("flow", flow)
    e.bp_set_evidence(ev)
    for _ in range(3):
        r = e.bp_run_device(1e-3)
    assert e.last_path() == 2
    n = 4096
    buf = np.zeros((n, 12), dtype=np.uint64)
    rc = L.bn_debug_tile_clock_resident(buf.ctypes.data_as(ctypes.c_void_p), n)
    assert rc == 0
    slot = np.flatnonzero(buf[:, 1] != 0)   # slot = block * 8 + wave: waves w and w + 4 of a block share a SIMD
    st = buf[slot].astype(np.int64)
    if not flow:   # a wave without a tile takes part in the barriers but never stamps the roles
        slot, st = slot[st[:, 7] != 0], st[st[:, 7] != 0]
    if flow:
        st[:, 5] = st[:, 4]  # no block-level arrival in the dataflow form
    t0 = st[:, 0].min()
    names = ["wait (neighbours / verdict)" if flow else "wait verdict", "parent role", "contraction", "normalise+stores issued", "drain", "block sync", "granules"]
    # order of the stamps in time: 0 start, 1 verdict, 7 parent role, 8 contraction, 3 sweep issued, 4 drained, 5 synced, 6 published
    order = [0, 1, 7, 8, 3, 4, 5, 6]
    d = np.stack([st[:, order[i + 1]] - st[:, order[i]] for i in range(len(order) - 1)], axis=1) * 10  # ns
    print(f"{rows}x{rows} grid, {'dataflow form' if flow else 'grid barrier'}, {r['sweeps']} sweeps, {st.shape[0]} waves stamped; iteration 6, ns: median / p90 / max over waves")
    for i, nm in enumerate(names):
        print(f"  {nm:26s} {np.median(d[:, i]):8.0f} {np.percentile(d[:, i], 90):8.0f} {d[:, i].max():8.0f}")
    tot = (st[:, 6] - st[:, 0]) * 10
    print(f"  {'iteration (start->published)':26s} {np.median(tot):8.0f} {np.percentile(tot, 90):8.0f} {tot.max():8.0f}")
    print("  spread of iteration starts over waves (ns):", (st[:, 0].max() - st[:, 0].min()) * 10, " of verdict arrival:", (st[:, 1].max() - st[:, 1].min()) * 10)
    print("  first start -> last publish (ns):", (st[:, 6].max() - t0) * 10)
    if not flow:
        # ---- the two halves of a block: waves 0-3 (dispatched first) and their SIMD partners 4-7; waves with a tile only (an idle
        # wave never stamps the roles).  Which half is the slow one, and in which phase?
        wave, blk = slot % 8, slot // 8
        tiled = st[:, 7] != 0
        release = np.full(blk.max() + 1, np.iinfo(np.int64).max)
        np.minimum.at(release, blk, st[:, 1])   # a block's release: the first of its waves to know the verdict
        halves = [("waves 0-3", tiled & (wave < 4)), ("waves 4-7", tiled & (wave >= 4))]
        phases = [("verdict known", 0, 1), ("parent role", 1, 7), ("contraction", 7, 8), ("normalise + stores", 8, 3), ("drain", 3, 4),
                  ("block sync", 4, 5), ("publish", 5, 6), ("compute: verdict -> sweep issued", 1, 3),
                  ("verdict -> stores drained", 1, 4)]
        print(f"  by half of the block, ns: median / p90 / max   {halves[0][0]} ({halves[0][1].sum()} waves) | {halves[1][0]} ({halves[1][1].sum()} waves)")
        for nm, i, j in phases:
            cells = []
            for _, m in halves:
                v = (st[m, j] - st[m, i]) * 10
                cells.append(f"{np.median(v):7.0f} {np.percentile(v, 90):7.0f} {v.max():7.0f}")
            print(f"    {nm:34s} {cells[0]}  | {cells[1]}")
        since = (st[:, 3] - release[blk]) * 10   # "sweep issued" since the block's release
        med = [np.median(since[m]) for _, m in halves]
        print(f"    {'sweep issued since block release':34s} " + "  | ".join(
            f"{np.median(since[m]):7.0f} {np.percentile(since[m], 90):7.0f} {since[m].max():7.0f}" for _, m in halves))
        print(f"  gap between the halves' medians at 'sweep issued' (waves 4-7 minus waves 0-3): {med[1] - med[0]:.0f} ns")
        # the collecting wave (wave 0 of every tile block, direct form): stamps 2 "every block's granule seen" and 9 "verdict written";
        # what stands between them is on every block's path, and the block's other waves are released behind the second (EXPERIMENTS R22)
        col = (wave == 0) & (st[:, 2] != 0) & (st[:, 9] != 0)
        if col.any():
            print(f"  collecting waves ({col.sum()}), ns: median / p90 / max")
            for nm, i, j in (("start -> poll returned", 0, 2), ("poll returned -> verdict written", 2, 9), ("verdict written -> released", 9, 1)):
                v = (st[col, j] - st[col, i]) * 10
                print(f"    {nm:34s} {np.median(v):7.0f} {np.percentile(v, 90):7.0f} {v.max():7.0f}")
            seen_last = st[col, 2].max()
            rel = (st[tiled, 1] - seen_last) * 10
            print(f"    last collector's poll returned -> a tile wave knows the verdict: {np.median(rel):.0f} median, {rel.max():.0f} max")
        comp = (st[:, 3] - st[:, 1]) * 10
        print("  compute (verdict -> sweep issued) by wave number, median ns:", " ".join(f"{np.median(comp[tiled & (wave == w)]):.0f}" for w in range(8)))
        slowest = np.argmax(np.where(tiled, comp, -1))
        print(f"  slowest wave's compute: {comp[slowest]} ns (block {blk[slowest]}, wave {wave[slowest]})")
        # per block: which half holds the wave that issues its sweep last, and how long the block's first four wait for it
        last_half = np.zeros(2, dtype=np.int64)
        wait = []
        for bk in np.unique(blk[tiled]):
            m = tiled & (blk == bk)
            if (m & (wave >= 4)).sum() == 0:
                continue
            w_last = wave[m][np.argmax(st[m, 3])]
            last_half[int(w_last >= 4)] += 1
            wait.append((st[m, 3].max() - np.median(st[m, 3])) * 10)
        print(f"  blocks whose last wave to issue is in waves 0-3 / waves 4-7: {last_half[0]} / {last_half[1]};"
              f" last wave behind the block's median wave, median over blocks: {np.median(wait):.0f} ns")
    # ---- the run's fixed cost: what is not sweeps (stamps of the LAST run above)
    run = np.zeros((n, 8), dtype=np.uint64)
    assert L.bn_debug_run_clock_resident(run.ctypes.data_as(ctypes.c_void_p), n) == 0
    rs = run[run[:, 0] != 0].astype(np.int64)
    assert (run[:, 6] == 0).all(), f"the recorder's re-read found a granule of another generation in iteration {int(run[:, 6].max()) - 1}"
    e0 = rs[:, 0].min()
    rows_ = [("entry -> CPT loads issued", rs[:, 1] - rs[:, 0]), ("entry -> CPT resident", rs[:, 2] - rs[:, 0]),
             ("CPT resident -> sweep 0 published", rs[:, 3] - rs[:, 2]), ("entry -> sweep 0 published", rs[:, 3] - rs[:, 0]),
             ("last verdict -> finalize stored", rs[:, 5] - rs[:, 4]), ("entry -> finalize stored", rs[:, 5] - rs[:, 0])]
    print(f"run-level stamps, {rs.shape[0]} waves, ns: median / p90 / slowest wave")
    for nm, v in rows_:
        v = v * 10
        print(f"  {nm:34s} {np.median(v):8.0f} {np.percentile(v, 90):8.0f} {v.max():8.0f}")
    print("  spread of kernel entries over waves (ns):", (rs[:, 0].max() - e0) * 10)
    print("  first entry -> last wave's CPT resident / sweep 0 published / last verdict / finalize stored (ns):",
          (rs[:, 2].max() - e0) * 10, (rs[:, 3].max() - e0) * 10, (rs[:, 4].max() - e0) * 10, (rs[:, 5].max() - e0) * 10)
    print("  sweeps 1.. : last sweep-0 publication -> last verdict (ns):", (rs[:, 4].max() - rs[:, 3].max()) * 10,
          f" = {(rs[:, 4].max() - rs[:, 3].max()) * 10 / max(r['sweeps'] - 1, 1):.0f} per sweep")
