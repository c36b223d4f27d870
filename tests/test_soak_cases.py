"""The soak's case generators (tests/soak_cases.py) without a device: they are pure functions of (leg, seed, index), every
`tables` case lies inside the library's input domain, the host references run clean and agree with each other on a sample of
the committed cases of every leg, the committed cases reach the paths and kernel forms tests/test_soak_gpu.py asserts, and the
oracle alone leaves at most 2 % of the small `bp` cases out of the sweep comparison."""
import dataclasses
import hashlib

import numpy as np
import pytest

import soak_cases as S


def fingerprint(x) -> str:
    """A digest of a case: arrays by dtype, shape and bytes, models and evidence by their fields."""
    h = hashlib.sha256()

    def feed(v):
        if dataclasses.is_dataclass(v) and not isinstance(v, type):
            feed({f.name: getattr(v, f.name) for f in dataclasses.fields(v)})
        elif isinstance(v, dict):
            for key in sorted(v):
                h.update(repr(key).encode())
                feed(v[key])
        elif isinstance(v, (list, tuple)):
            h.update(f"[{len(v)}".encode())
            for item in v:
                feed(item)
        elif isinstance(v, np.ndarray):
            h.update(f"{v.dtype}{v.shape}".encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    feed(x)
    return h.hexdigest()


def committed(leg, step=1):
    return [S.make_case(leg, S.SUITE[leg]["seed"], i) for i in range(0, S.SUITE[leg]["cases"], step)]


@pytest.mark.parametrize("leg", sorted(S.LEGS))
def test_a_case_is_a_function_of_its_key(leg):
    seed = S.SUITE[leg]["seed"]
    alone = fingerprint(S.make_case(leg, seed, 5))
    after_others = [fingerprint(S.make_case(leg, seed, i)) for i in (3, 4, 5)]
    assert after_others[2] == alone and fingerprint(S.make_case(leg, seed, 5)) == alone
    others = {alone, after_others[0], after_others[1], fingerprint(S.make_case(leg, seed + 1, 5))}
    others |= {fingerprint(S.make_case(other, seed, 5)) for other in S.LEGS if other != leg}
    assert len(others) == 4 + len(S.LEGS) - 1
    case = S.make_case(leg, seed, 5)
    assert S.parse_key(case["key"]) == (leg, seed, 5) and case["key"] == S.case_key(leg, seed, 5)
    with pytest.raises(ValueError):
        S.parse_key("nothing:1:2")


def test_chunks_cover_every_committed_index_once():
    for leg in S.LEGS:
        covered = [i for a, b in S.suite_chunks(leg) for i in range(a, b)]
        assert covered == list(range(S.SUITE[leg]["cases"]))


def test_every_tables_case_is_inside_the_input_domain():
    for seed, count in ((S.SUITE["tables"]["seed"], S.SUITE["tables"]["cases"]), (7, 150)):
        for index in range(count):
            case = S.tables_case(seed, index)
            assert S.tables_domain_ok(case), case["key"]
            assert 3 <= len(case["k"]) <= 40 and 1 <= case["k"].min() and case["k"].max() <= 255
            assert all(len(cand) <= 12 for _, _, cand in case["lattices"])
            assert (case["search"] is not None) == (len(case["k"]) <= S.SEARCH_COLUMNS)
            assert all(c in case["pair_cols"] and u in case["pair_cols"] and c != u for c, u in case["cross"])


def test_the_committed_tables_cases_reach_every_form():
    forms = [S.tables_forms(case) for case in committed("tables")]
    for name in ("count_lds", "count_global", "lattice_lds", "lattice_levels", "multi_chunk", "digit_passes>1", "arity1_child",
                 "arity1_parent", "lattice_arity1_top_digit", "zero_weights", "search"):
        assert any(name in f for f in forms), name


def test_group_chunks_follows_the_chunking_rule():
    k = [2] * 40 + [255, 255, 16]
    assert S.group_chunks(k, (0, [], [])) == 1
    assert S.group_chunks(k, (0, [1], list(range(2, 34)))) == 1           # 32 candidates of 8 cells: one LDS chunk
    assert S.group_chunks(k, (0, [1], list(range(2, 35)))) == 2           # the 33rd opens another
    assert S.group_chunks(k, (0, list(range(1, 10)), [10, 11, 12])) == 2  # 1 024 + 3 x 2 048 cells: over one block of 4 096
    assert S.group_chunks(k, (40, [41], [0, 1])) == 1                     # device memory: up to 8 candidates
    assert S.group_chunks(k, (40, [41], list(range(9)))) == 2
    assert S.group_chunks(k, (42, [0], [40, 41, 1])) == 2                 # small and large families never share a chunk


def test_the_host_references_agree_on_a_sample_of_tables_cases():
    for case in committed("tables", step=6):
        S.check_tables_host(case)


def test_the_oracle_runs_clean_on_a_sample_of_sampler_cases(oracle_mod):
    ran = 0
    for case in committed("samplers", step=2):
        if case["n"] > 600:
            continue
        g, ns = case["g"], min(case["ns"], 1000)
        o = oracle_mod.lw_run(g, case["st"], ns, seed=case["seed"], s_begin=case["begin"], states_cap=ns)
        assert (o["states"] < g.k[None, :]).all() and (o["weights"] >= 0).all() and np.isfinite(o["hist"]).all(), case["key"]
        fixed = case["st"] >= 0
        assert (o["states"][:, fixed] == case["st"][fixed]).all(), case["key"]
        per_node = np.add.reduceat(o["hist"], g.node_off[:-1])
        assert np.allclose(per_node, o["weights"].sum(), rtol=1e-9), case["key"]
        pats, counts = np.unique(o["states"], axis=0, return_counts=True)
        cpt = oracle_mod.make_cpt(g, pats, counts)
        rows = np.add.reduceat(cpt, np.concatenate([np.arange(g.cpt_off[v], g.cpt_off[v + 1], g.k[v]) for v in range(g.n)]))
        assert np.allclose(rows, 1.0, rtol=1e-12), case["key"]
        ran += 1
    assert ran >= 5


def test_the_oracle_alone_leaves_out_at_most_two_percent_of_the_small_bp_cases(oracle_mod):
    cases = [c for c in committed("bp") if c["g"].n <= 500]
    assert len(cases) >= 50
    left_out = []
    for case in cases:
        want = S.bp_oracle(case, oracle_mod, S.oracle_threads(case))
        assert want["sweeps"] >= 1 and len(want["residuals"]) == min(want["sweeps"], 4096), case["key"]
        if S.bp_left_out_by_oracle(case, want):
            left_out.append(case["key"])
    assert len(left_out) <= S.LEFT_OUT_SHARE * len(cases), left_out


def test_the_committed_bp_cases_hold_what_the_coverage_conditions_need():
    cases = committed("bp")
    assert sum(c["batch_seeds"] is not None for c in cases) >= 100
    assert any(c["shards"] is not None and c["shards"]["owner"] is not None for c in cases)
    assert any(c["shards"] is not None and c["shards"]["owner"] is None for c in cases)
    assert any(c["beyond_launch"] for c in cases) and any(c["zero_evidence"] for c in cases)
    assert any(c["reload_seed"] is not None for c in cases) and any(c["lw"] is not None for c in cases)
    assert {c["eps"] for c in cases} >= {1e-3, 1e-6, 1e-9, 0.0}
    assert all(c["shards"] is None or 2 <= c["shards"]["nranks"] <= 5 for c in cases)
