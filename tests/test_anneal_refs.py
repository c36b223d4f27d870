"""CPU-only: the restatements tests/test_anneal_gpu.py rests on (tests/anneal_refs.py).  The index is a bijection; the restated
chain (what the kernel does) equals the literal transcription of the reference's loop in every record and every trace entry on
every fixed input the GPU tests use; and those inputs reach every branch of the loop."""
from math import comb

import pytest

import anneal_refs as AR

RECORD = ("eval", "proposals", "operated", "accepted", "flags", "masks", "edges", "trace", "uphill")


@pytest.mark.parametrize("n,q", [(1, 1), (2, 1), (5, 2), (6, 5), (33, 3), (64, 2), (4, 3)])
def test_rank_and_unrank_are_a_bijection(n, q):
    T = AR.row_entries(n, q)
    assert T == sum(comb(n - 1, t) for t in range(q + 1))
    for child in sorted({0, n // 2, n - 1}):
        seen = set()
        for r in range(T):
            S = AR.unrank(n, q, child, r)
            assert len(S) <= q and child not in S and all(0 <= u < n for u in S) and S == sorted(set(S))
            assert AR.rank(n, child, S) == r
            seen.add(tuple(S))
        assert len(seen) == T


def test_row_sizes_the_header_names():
    assert (AR.row_entries(37, 3), AR.row_entries(64, 3), AR.row_entries(37, 4)) == (7807, 41728, 66712)


def test_stream_is_the_samplers():
    """stream_seed of oracle/lw_oracle.c: Philox4x32-10 on ({j_lo, j_hi, 0, 0}, {seed_lo, seed_hi}); the Random123 known answers."""
    assert AR.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert AR.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    s = AR.Stream(5, 7)
    assert s.x == AR.philox4x32_10((7, 0, 0, 0), (5, 0))
    draws = [s.below(3) for _ in range(300)]
    assert set(draws) == {0, 1, 2}
    assert all(0.0 < AR.Stream(1, j).uniform() < 1.0 for j in range(50))


_EVENTS = {}
_LONGEST = {}


@pytest.mark.parametrize("name", list(AR.RUNS))
def test_restated_chain_equals_the_literal_transcription(name):
    pb, sched, chains, seed = AR.run_setup(name)
    events = _EVENTS.setdefault(name, {})
    for j in range(chains):
        lit = AR.literal_chain(pb, sched, seed, j)
        res = AR.restated_chain(pb, sched, seed, j, events)
        for key in RECORD:
            assert lit[key] == res[key], (name, j, key)
        _LONGEST[name] = max(_LONGEST.get(name, 0), res["longest_list"])
        assert AR.exp_margin_ok(res["uphill"]), (name, j)   # (the GPU test's precondition, here over libm's terms)
        # the restated terms and parameter count are those of the final graph
        assert res["eval"] == pb.score([pb.term(v, AR._parents_of(res["masks"][v])) for v in range(pb.n)], res["params"])


def _events_by_rule():
    total = {"reference": {}, "metropolis": {}}
    for name in AR.RUNS:
        if name not in _EVENTS or name not in _LONGEST:   # (run alone: fill in)
            pb, sched, chains, seed = AR.run_setup(name)
            _EVENTS[name] = {}
            for j in range(chains):
                _LONGEST[name] = max(_LONGEST.get(name, 0), AR.restated_chain(pb, sched, seed, j, _EVENTS[name])["longest_list"])
        for key, count in _EVENTS[name].items():
            rule = total[AR.RUNS[name][3]]
            rule[key] = rule.get(key, 0) + count
    return total


def test_the_fixed_inputs_reach_every_branch():
    total = _events_by_rule()
    both = ("add_accepted", "refused_self", "refused_existing", "refused_cycle", "refused_q", "delete_operated", "no_edges",
            "reverse_operated", "reverse_refused_moved", "downhill_accept", "uphill_accept", "uphill_reject", "end_temperature")
    for rule, seen in total.items():
        missing = [key for key in both if not seen.get(key)]
        assert not missing, (rule, missing, seen)
    seen = {key: total["reference"].get(key, 0) + total["metropolis"].get(key, 0) for key in set(total["reference"]) | set(total["metropolis"])}
    for key in ("end_same_state", "end_cap", "refused_nan"):
        assert seen.get(key), (key, seen)
    assert _EVENTS["n1_cap"] == {"refused_self": _EVENTS["n1_cap"].get("refused_self", 0), "no_edges": _EVENTS["n1_cap"].get("no_edges", 0),
                                 "end_cap": 1}


def test_the_fixed_inputs_reach_every_long_list_form():
    """What the kernel does 64 entries at a time: an erase with more than 64 (one more round) and more than 128 (two more) entries
    behind the erased one, accept and reject copies of more than 64 entries, and a refused reversal that reorders such a list --
    each under BOTH rules (erase_tail_gt128 too: no exception is taken).  The longest list holds every edge of the 186-edge start;
    the bounded run refuses at in-degree 2 over the q = 3 table; the long chains end by temperature after thousands of uphill
    decisions."""
    total = _events_by_rule()
    for rule, seen in total.items():
        missing = [key for key in ("erase_tail_gt64", "erase_tail_gt128", "copy_gt64_accept", "copy_gt64_reject", "reverse_refused_moved_gt64")
                   if not seen.get(key)]
        assert not missing, (rule, missing, seen)
    assert max(_LONGEST.values()) >= 180 and _LONGEST["n64_dense_met"] >= 180 and _LONGEST["n64_dense_ref"] >= 180
    assert _LONGEST["n33_dense_ref"] > 64
    bounded = _EVENTS["n33_bound2_over_q3"]
    assert AR.MAX_PARENTS["n33_bound2_over_q3"] == 2 < AR.RUNS["n33_bound2_over_q3"][1] and bounded.get("refused_q", 0) > 0
    assert all(len(p) <= 2 for p in AR.RUNS["n33_bound2_over_q3"][12]) and any(len(p) == 2 for p in AR.RUNS["n33_bound2_over_q3"][12])
    for name in ("n33_dense_ref", "n5_long_met", "n6_long_ref"):
        assert _EVENTS[name].get("end_temperature") == AR.RUNS[name][10] and not _EVENTS[name].get("end_same_state"), name
    for name in ("n5_long_met", "n6_long_ref"):
        assert _EVENTS[name]["uphill_accept"] + _EVENTS[name]["uphill_reject"] > 5000, name
