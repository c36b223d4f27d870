#!/usr/bin/env python3
"""Which execution path an engine takes, and what it reports as eligible, for a fixed list of networks under the defaults and under
each FORCE set of scripts/time_paths.py: the table tests/test_path_choice_gpu.py compares every later build against
(tests/golden/path_choice.json).  One bn_bp_run_device with max_sweeps = 2 on 2 % random evidence per entry.  GPU box only:
    python scripts/record_path_choice.py [out.json]        (BN_MI355X_LIB selects the build that is recorded)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bayesiannetwork_amd import synth  # noqa: E402
from bayesiannetwork_amd.dsc import load_dsc  # noqa: E402
from bayesiannetwork_amd.engine import Engine  # noqa: E402
from time_paths import DEFAULTS, FORCE  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "path_choice.json")
INFOS = ("last_flow", "last_dag_flow", "resident_eligible", "resident_blocks", "resident_waves", "flow_eligible", "small_eligible",
         "mid_eligible", "mid_parts", "dag_eligible", "dag_blocks", "dag_stream")
CONFIGS = [("default", {})] + [(f"force{path}", opts) for path, opts in FORCE.items()]


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


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    table = {"n_cus": device_cus(), "networks": {name: entries_of(g) for name, g in networks()}}
    with open(out_path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, rows in table["networks"].items():
        print(f"{name:16s} " + "  ".join(f"{c}: {r['last_path']}" for c, r in rows.items()))


if __name__ == "__main__":
    main()
