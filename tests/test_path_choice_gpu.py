"""Which execution path an engine takes and what it reports as eligible, for fifteen networks under the defaults and under every
FORCE set of scripts/time_paths.py, against the table scripts/record_path_choice.py recorded on an MI355X
(tests/golden/path_choice.json) before the choice became bn_engine_policy.cpp: every entry must be equal.  The table belongs to a
device of its CU count (the resident launch shape, the 0.9 x CUs caps): on another count the test skips."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_path_choice", os.path.join(ROOT, "scripts", "record_path_choice.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_path_choice_equals_the_recorded_table():
    rec = _recorder()
    with open(rec.GOLDEN) as f:
        golden = json.load(f)
    cus = rec.device_cus()
    if cus != golden["n_cus"]:
        pytest.skip(f"the table was recorded on a device of {golden['n_cus']} CUs, this one has {cus}")
    nets = rec.networks()
    assert sorted(name for name, _ in nets) == sorted(golden["networks"])
    differing = []
    for name, g in nets:
        got, want = rec.entries_of(g), golden["networks"][name]
        assert sorted(got) == sorted(want)
        for config in want:
            for key, value in want[config].items():
                if got[config].get(key) != value:
                    differing.append(f"{name} {config} {key}: {got[config].get(key)} (recorded {value})")
            assert sorted(got[config]) == sorted(want[config])
    assert not differing, "\n".join(differing)


def test_every_batch_path_choice_equals_the_recorded_table():
    """Which path a BATCH of 1, 2, 5 and (networks of at most 5 000 nodes) 17 evidence sets takes, how many launches it needs and
    whether it ran on the second, dense engine, against tests/golden/batch_path_choice.json -- recorded before the batch policy, the
    chunk arithmetic and the staging layout became pure host functions (from the parent's sources with the one assignment of
    EXPERIMENTS R18.1 added: without it the recording itself reads a stale staging block): every entry must be equal."""
    rec = _recorder()
    with open(rec.BATCH_GOLDEN) as f:
        golden = json.load(f)
    cus = rec.device_cus()
    if cus != golden["n_cus"]:
        pytest.skip(f"the table was recorded on a device of {golden['n_cus']} CUs, this one has {cus}")
    nets = rec.networks()
    assert sorted(name for name, _ in nets) == sorted(golden["networks"])
    differing = []
    for name, g in nets:
        got, want = rec.batch_entries_of(name, g), golden["networks"][name]
        assert sorted(got) == sorted(want)
        for config in want:
            assert sorted(got[config]) == sorted(want[config]), (name, config)
            for size, row in want[config].items():
                if got[config][size] != row:
                    differing.append(f"{name} {config} {size}: {got[config][size]} (recorded {row})")
    assert not differing, "\n".join(differing)
