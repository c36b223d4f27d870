#!/usr/bin/env python3
"""Which execution path an engine takes, and what it reports as eligible, for a fixed list of networks under the defaults and under
each FORCE set of scripts/time_paths.py: the table tests/test_path_choice_gpu.py compares every later build against
(tests/golden/path_choice.json).  One bn_bp_run_device with max_sweeps = 2 on 2 % random evidence per entry.  GPU box only:
    python scripts/record_path_choice.py [out.json]        (BN_MI355X_LIB selects the build that is recorded)

A second table pins which path a BATCH takes and how many launches it needs (tests/golden/batch_path_choice.json): the same networks
and option sets, batches of 1, 2 and 5 sets (5 is more than one resident launch walks: chunks of 3 and 2) and, on networks of at most
5 000 nodes, of 17 (one more than a launch of the register-resident DAG kernel holds); set q carries 2 % random evidence of seed
7 + q, every entry is bn_bp_set_evidence_batch + bn_bp_run_batch_device(1e-6, 2).  Every network runs every size: the whole table
takes 2.3 s on an MI355X, so no grid is left out of the 5-set column.  An entry the library answers with an error would be pinned
as that error; the table has none.
    python scripts/record_path_choice.py --batch [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bayesiannetwork_amd import synth  # noqa: E402
from bayesiannetwork_amd._lib import BnError  # noqa: E402
from bayesiannetwork_amd.dsc import load_dsc  # noqa: E402
from bayesiannetwork_amd.engine import Engine  # noqa: E402
from time_paths import DEFAULTS, FORCE  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "path_choice.json")
INFOS = ("last_flow", "last_dag_flow", "resident_eligible", "resident_blocks", "resident_waves", "flow_eligible", "small_eligible",
         "mid_eligible", "mid_parts", "dag_eligible", "dag_blocks", "dag_stream")
CONFIGS = [("default", {})] + [(f"force{path}", opts) for path, opts in FORCE.items()]
BATCH_GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_path_choice.json")
BATCH_SIZES = (1, 2, 5)
BATCH_SIZE_SMALL_NETS = 17      # kDagMaxSets + 1 ...
BATCH_SMALL_NET_NODES = 5000    # ... on networks of at most this many nodes
BATCH_SKIP = {}                 # {network name: sizes left out} (none)


def networks():
    alarm, _ = load_dsc(os.path.join(ROOT, "tests", "golden", "alarm_shaped.dsc"))
    nets = [("pearl", synth.pearl()), ("alarm_shaped", alarm)]
    for r, c in ((8, 8), (16, 16), (40, 40), (64, 64), (160, 160), (200, 200), (239, 240), (316, 316)):
        nets.append((f"grid{r}x{c}_k4", synth.grid(r, c, 4, seed=1)))
    nets += [("grid128x128_k2", synth.grid(128, 128, 2, seed=1)), ("chain200", synth.grid(200, 1, 4, seed=5)),
             ("mixed60", synth.random_dag(60, 3, 16, [2, 3, 4, 3, 2, 4, 4], seed=9)),
             ("dag200", synth.random_dag(200, 4, 64, 4, seed=200)), ("dag2p_3000", synth.random_dag(3000, 2, 64, 4, seed=3))]
    return nets


def entries_of(g):
    """{config name: {"last_path": ..., every name of INFOS: ...}} of one network, every configuration on the same engine."""
    out = {}
    ev = synth.random_evidence(g, 0.02, seed=7)
    with Engine(g) as eng:
        eng.bp_set_evidence(ev)
        for name, opts in CONFIGS:
            for k, v in {**DEFAULTS, **opts}.items():
                eng.set_option(k, v)
            eng.bp_run_device(1e-6, 2)
            row = {"last_path": eng.last_path()}
            row.update({i: eng.info(i) for i in INFOS})
            out[name] = row
    return out


def batch_sizes_of(name, g):
    sizes = BATCH_SIZES + ((BATCH_SIZE_SMALL_NETS,) if g.n <= BATCH_SMALL_NET_NODES else ())
    return tuple(b for b in sizes if b not in BATCH_SKIP.get(name, ()))


def batch_entries_of(name, g):
    """{config name: {"b<sets>": {"last_path", "sweep_launches", "batch_on_dense", "batch_dense_refused"}}} of one network, every
    configuration and batch size on the same engine."""
    out = {}
    sizes = batch_sizes_of(name, g)
    evs = [synth.random_evidence(g, 0.02, seed=7 + q) for q in range(max(sizes))]
    with Engine(g) as eng:
        for config, opts in CONFIGS:
            for k, v in {**DEFAULTS, **opts}.items():
                eng.set_option(k, v)
            rows = out[config] = {}
            for b in sizes:
                eng.bp_set_evidence_batch(evs[:b])
                try:
                    eng.bp_run_batch_device(1e-6, 2)
                except BnError as ex:   # (an entry the library answers with an error is pinned as that error)
                    print(f"{name} {config} b{b}: {ex}")
                    rows[f"b{b}"] = {"error": ex.code}
                    continue
                rows[f"b{b}"] = {"last_path": eng.last_path(), "sweep_launches": eng.bp_stats()["sweep_launches"],
                                 "batch_on_dense": eng.info("batch_on_dense"), "batch_dense_refused": eng.info("batch_dense_refused")}
    return out


def record_batches(out_path):
    t0 = time.perf_counter()
    table = {"n_cus": device_cus(), "networks": {}}
    for name, g in networks():
        t1 = time.perf_counter()
        rows = table["networks"][name] = batch_entries_of(name, g)
        print(f"{name:16s} {time.perf_counter() - t1:5.2f} s  " +
              "  ".join(f"{c}: " + "/".join(f"{r.get('last_path', 'E')}x{r.get('sweep_launches', '')}" for r in by.values()) for c, by in rows.items()))
    with open(out_path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"batch table: {time.perf_counter() - t0:.1f} s wall (networks built, engines created, every batch run)")


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--batch":
        return record_batches(sys.argv[2] if len(sys.argv) > 2 else BATCH_GOLDEN)
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    table = {"n_cus": device_cus(), "networks": {name: entries_of(g) for name, g in networks()}}
    with open(out_path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, rows in table["networks"].items():
        print(f"{name:16s} " + "  ".join(f"{c}: {r['last_path']}" for c, r in rows.items()))


if __name__ == "__main__":
    main()
