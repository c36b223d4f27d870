"""The randomised parity soaks in the GPU suite: the three legs of tests/soak_cases.py with the seeds and case counts fixed there,
in chunks of consecutive indices -- a failure names its chunk, its message the case (`leg:seed:index`), and
`python scripts/soak_gpu.py --case leg:seed:index` replays exactly that case.  A last test per leg asserts that the leg took the
paths and kernel forms it is there for, so the file cannot pass hollow.

bp: a sweep count is compared only where the oracle's residual history stays clear of eps (soak_cases.bp_margins); a case where
it does not is left out of the sweep comparison and counted, and at most 2 % of the cases may be.  Nothing else is skipped."""
import time

import pytest

import soak_cases as S

pytestmark = pytest.mark.gpu

RECORDS = {leg: {} for leg in S.LEGS}


def run_chunk(leg, first, last, *modules):
    seed = S.SUITE[leg]["seed"]
    for index in range(first, last):
        t0 = time.time()
        case = S.make_case(leg, seed, index)
        rec = S.CHECKS[leg](case, *modules)
        RECORDS[leg][index] = rec
        print(f"{S.LINES[leg](case, rec)}  [{rec['comparisons']} comparisons, {time.time() - t0:.2f} s]")


def whole_leg(leg):
    recs = RECORDS[leg]
    assert len(recs) == S.SUITE[leg]["cases"], f"{leg}: {len(recs)} of {S.SUITE[leg]['cases']} cases ran; the coverage conditions need every chunk"
    return list(recs.values())


@pytest.mark.parametrize("first,last", S.suite_chunks("bp"))
def test_bp_cases(bnlib, oracle_mod, first, last):
    from bayesiannetwork_amd import engine
    run_chunk("bp", first, last, engine, oracle_mod)


def test_bp_leg_took_every_path(bnlib):
    recs = whole_leg("bp")
    taken = {p: sum(p in r["paths"] for r in recs) for p in (0, 2, 3, 4, 5, "5f")}
    batch, left_out = sum(r["batch"] for r in recs), sum(r["left_out"] for r in recs)
    print(f"bp: {len(recs)} cases, {sum(r['comparisons'] for r in recs)} comparisons; forced paths {taken}; batch in {batch}; shards "
          f"{[r['shards'] for r in recs if r['shards']]}; beyond one launch {sum(r['beyond_launch'] for r in recs)}; all-zero evidence "
          f"{sum(r['zero_evidence'] for r in recs)}; reload {sum(r['reload'] for r in recs)}; likelihood weighting {sum(r['lw'] for r in recs)}; "
          f"left out of the sweep comparison {left_out}")
    assert all(count >= 10 for count in taken.values()), taken
    assert batch >= 100, batch
    assert any(r["shards"] == "owner map" for r in recs)
    assert any(r["beyond_launch"] for r in recs)
    assert any(r["zero_evidence"] for r in recs)
    assert left_out <= S.LEFT_OUT_SHARE * len(recs), f"{left_out} of {len(recs)} bp cases were left out of the sweep comparison"


@pytest.mark.parametrize("first,last", S.suite_chunks("samplers"))
def test_sampler_cases(bnlib, oracle_mod, first, last):
    from bayesiannetwork_amd import engine
    run_chunk("samplers", first, last, engine, oracle_mod)


def test_samplers_leg_took_both_kernels(bnlib):
    recs = whole_leg("samplers")
    kernels = {name: sum(r["kernel"] == name for r in recs) for name in ("straight-line", "generic")}
    print(f"samplers: {len(recs)} cases, {sum(r['comparisons'] for r in recs)} comparisons; kernels {kernels}; rejection sampling "
          f"{sum(r['rs'] for r in recs)}; fit_cpt {sum(r['fit'] for r in recs)}")
    assert all(kernels.values()), kernels
    assert any(r["rs"] for r in recs) and any(r["fit"] for r in recs)


@pytest.mark.parametrize("first,last", S.suite_chunks("tables"))
def test_table_cases(bnlib, first, last):
    import bayesiannetwork_amd
    run_chunk("tables", first, last, bayesiannetwork_amd)


def test_tables_leg_took_every_form(bnlib):
    recs = whole_leg("tables")
    names = ("count_lds", "count_global", "lattice_lds", "lattice_levels", "multi_chunk", "digit_passes>1", "arity1_child", "arity1_parent",
             "lattice_arity1_top_digit", "zero_weights", "search")
    forms = {name: sum(name in r["forms"] for r in recs) for name in names}
    print(f"tables: {len(recs)} cases, {sum(r['comparisons'] for r in recs)} comparisons; forms {forms}")
    assert all(forms.values()), forms
    assert any(r["digit_passes"] > 1 for r in recs)
