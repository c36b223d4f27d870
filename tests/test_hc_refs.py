"""CPU: the restated hierarchical-clustering search (tests/hc_refs.py, what the kernel does) equals the literal transcription of
the reference's loop, and the three facts that let the restated form and the kernel drop steps hold on the literal form."""
import math

import numpy as np
import pytest

import anneal_refs as AR
import hc_refs as HR

SAME = ("score", "merges", "tried", "kept", "pruned", "pairs_kept", "flags", "masks", "merge_trace", "prune_trace", "decisions",
        "sims", "clusters")


def assert_same(lit, res, what):
    for key in SAME:
        a, b = lit[key], res[key]
        if key in ("score",):
            a, b = HR.bits(a), HR.bits(b)
        if key == "decisions":
            a, b = [(HR.bits(u), HR.bits(p)) for u, p in a], [(HR.bits(u), HR.bits(p)) for u, p in b]
        assert a == b, (what, key)


def assert_facts(lit, what):
    f = lit["facts"]
    assert f["sweep_removed"] == 0, what          # the closing sweep never removes anything
    assert f["refused_cycle"] == 0 and f["refused_existing"] == 0, what
    assert f["sims_over"] == 0, what              # len(sims) <= C(live clusters, 2)


@pytest.mark.parametrize("name", list(HR.RUNS))
def test_literal_equals_restated_on_the_fixed_runs(name):
    pb, S, alpha, runs, seed = HR.run_setup(name)
    if name == "n64":
        runs = 2   # (the literal form walks the graph per candidate; the GPU test replays all eight restated runs)
    for j in range(runs):
        lit, res = HR.literal_run(pb, S, alpha, seed, j), HR.restated_run(pb, S, alpha, seed, j)
        assert_same(lit, res, (name, j))
        assert_facts(lit, (name, j))


@pytest.mark.parametrize("name", list(HR.RUNS))
def test_every_fixed_seed_keeps_its_pruning_decisions_off_the_threshold(name):
    pb, S, alpha, runs, seed = HR.run_setup(name)
    for j in range(runs):
        res = HR.restated_run(pb, S, alpha, seed, j)
        assert HR.pow_margin_ok(res["decisions"], alpha, res["exponents"]), (name, j)


def random_case(rng):
    n = int(rng.integers(1, 9))
    k = [int(x) for x in rng.integers(1, 4, n)]
    q = int(rng.integers(1, 4))
    cache = {}
    nan_rate = float(rng.choice([0.0, 0.0, 0.15]))
    salt = int(rng.integers(1 << 30))

    def term(child, parents):
        key = (child, tuple(parents))
        if key not in cache:
            g = np.random.default_rng([salt, child, sum(1 << u for u in parents)])
            cache[key] = math.nan if parents and g.random() < nan_rate else -float(g.random()) * 40 - 3.0 / (1 + len(parents))
        return cache[key]

    kind = int(rng.integers(5))
    S = np.zeros((n, n))
    for x in range(n):
        for y in range(x + 1, n):
            if kind == 0:
                v = float(rng.random())
            elif kind == 1:
                v = float(rng.integers(0, 3)) * 0.25           # ties and exact zeros
            elif kind == 2:
                v = float(rng.normal())                        # negative entries
            elif kind == 3:
                v = 0.0
            else:
                v = float(rng.choice([math.nan, math.inf, 0.5, 1.0, -math.inf]))
            S[x][y] = S[y][x] = v
    alpha = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0, 2.0]))
    return AR.Problem(k, q, str(rng.choice(["aic", "mdl"])), int(rng.integers(10, 5000)), term), S, alpha


def test_literal_equals_restated_on_random_small_cases():
    rng = np.random.default_rng(20240)
    events = {}
    visits = {0: 0, 1: 0, 2: 0}
    for case in range(3000):
        pb, S, alpha = random_case(rng)
        seed, j = int(rng.integers(1 << 40)), int(rng.integers(4))
        lit, res = HR.literal_run(pb, S, alpha, seed, j), HR.restated_run(pb, S, alpha, seed, j, events)
        assert_same(lit, res, case)
        assert_facts(lit, case)
        assert lit["facts"]["refused_q"] == events.get("refused_q", 0) - visits.get("q", 0)
        assert lit["facts"]["refused_nan"] == events.get("refused_nan", 0) - visits.get("nan", 0)
        visits["q"], visits["nan"] = events.get("refused_q", 0), events.get("refused_nan", 0)
    # every branch was reached
    assert all(events.get(name, 0) > 0 for name in ("refused_q", "refused_nan", "visit_0", "visit_1", "visit_2")), events


def test_the_draw_order_of_a_merge():
    """The coin, the child shuffle, per child its parent shuffle, then one uniform per surviving cluster with a connection."""
    pb, S, alpha, runs, seed = HR.run_setup("n5_mid")
    for j in range(runs):
        lit = HR.literal_run(pb, S, alpha, seed, j)
        draws, at = lit["draws"], 0
        sizes = {i: 1 for i in range(pb.n)}
        visits = iter(lit["prune_trace"])
        live = pb.n
        for s, (parent, child, _, _) in enumerate(lit["merge_trace"]):
            assert draws[at] == "coin" and draws[at + 1] == ("children", sizes[child])
            at += 2
            for _ in range(sizes[child]):
                assert draws[at] == ("parents", sizes[parent])
                at += 1
            sizes[pb.n + s] = sizes[parent] + sizes[child]
            live -= 1
            for _ in range(live - 1):
                if next(visits)[1] > 0:
                    assert draws[at] == "uniform"
                    at += 1
        assert at == len(draws)
        # the stream is consumed exactly so: the step that many draws lead to is the run's last uniform
        if draws and draws[-1] == "uniform":
            steps = sum(1 if d in ("coin", "uniform") else max(d[1] - 1, 0) for d in draws)
            g = AR.Stream(seed, j)
            for _ in range(steps - 1):
                g.next()
            assert g.uniform() == lit["decisions"][-1][0]


def lane_strided_pick(values):
    """The pick as 64 lanes make it: per lane the first largest key of its strided entries, then a butterfly over the lanes in
    which the larger key wins and, among equal keys, the lower index."""
    lanes = []
    for lane in range(64):
        best, best_key = None, 0.0
        for i in range(lane, len(values), 64):
            v = values[i]
            key = (math.inf if i == 0 else -math.inf) if v != v else v
            if best is None or key > best_key:
                best, best_key = i, key
        lanes.append((best, best_key))
    off = 32
    while off >= 1:
        merged = []
        for lane in range(64):
            (best, best_key), (other, other_key) = lanes[lane], lanes[lane ^ off]
            if other is not None and (best is None or other_key > best_key or (other_key == best_key and other < best)):
                best, best_key = other, other_key
            merged.append((best, best_key))
        lanes, off = merged, off >> 1
    assert len({b for b, _ in lanes}) == 1
    return lanes[0][0]


def test_first_maximum_takes_the_first_of_equal_maxima_and_treats_nan_as_the_loop_does():
    assert HR.first_maximum([1.0, 3.0, 3.0, 2.0]) == 1 == HR.first_maximum_keyed([1.0, 3.0, 3.0, 2.0])
    assert HR.first_maximum([0.5, 0.5, 0.5]) == 0 == HR.first_maximum_keyed([0.5, 0.5, 0.5])
    nan, inf = math.nan, math.inf
    for values in ([nan, 1.0, inf], [1.0, nan, 2.0, 2.0], [-inf, nan], [nan, nan], [1.0, nan], [-inf, nan, -inf], [0.0, -0.0], [-0.0, 0.0]):
        assert HR.first_maximum(values) == HR.first_maximum_keyed(values), values
    rng = np.random.default_rng(7)
    for _ in range(2000):
        values = [float(x) for x in rng.choice([nan, inf, -inf, 0.0, 0.25, 0.5, 1.0], int(rng.integers(1, 12)))]
        assert HR.first_maximum(values) == HR.first_maximum_keyed(values), values
    # the kernel's form of the pick on lists of more than 64 entries: lane l takes the first maximum of the entries l, l + 64, ...
    # (a later one replaces it only when strictly larger), then the lanes are merged pairwise, the lower index winning among equal
    # keys.  With repeated maxima and +-inf it must give the index of std::max_element.
    for _ in range(1500):
        m = int(rng.integers(65, 301))
        pool = [[inf, -inf, 0.25, 0.5], [inf, nan, 0.5], [-inf, nan], [0.5], [0.25, 0.5, 1.0, -0.375, 0.0, -0.0]][int(rng.integers(5))]
        values = [float(x) for x in rng.choice(pool, m)]
        top = float(rng.choice([inf, 1.0, 2.0]))
        for i in rng.choice(m, int(rng.integers(2, 6)), replace=False):   # repeated maxima (or, under +inf in the pool, more of them)
            values[int(i)] = top
        want = HR.first_maximum(values)
        assert HR.first_maximum_keyed(values) == want, values
        assert lane_strided_pick(values) == want, values
        keys = [(inf if i == 0 else -inf) if v != v else v for i, v in enumerate(values)]
        assert keys.count(keys[want]) >= 2 or values[0] != values[0]
    # in a run: a caller's matrix of two values, the first pair in row-major order that holds the larger is merged first
    pb, S, alpha, runs, seed = HR.run_setup("n5_ties")
    res = HR.restated_run(pb, S, alpha, seed, 0)
    parent, child, value_bits, coin = res["merge_trace"][0]
    assert {parent, child} == {0, 2} and value_bits == HR.bits(0.5) and (parent, child) == ((2, 0) if coin else (0, 2))


def test_the_edge_cases_the_gpu_test_relies_on():
    def runs_of(name):
        pb, S, alpha, runs, seed = HR.run_setup(name)
        return pb, [HR.restated_run(pb, S, alpha, seed, j) for j in range(runs)]

    pb, out = runs_of("t1")
    assert all(r["merges"] == 0 and r["flags"] & HR.NO_SIMILARITY and r["score"] == pb.score([pb.term(0, ())], pb.k[0] - 1) for r in out)
    pb, out = runs_of("t2")
    assert all(r["merges"] == 1 and r["prune_trace"] == [] for r in out)
    pb, out = runs_of("t3")
    assert all(r["prune_trace"][0][1] == 2 and r["merges"] == (1 if r["prune_trace"][0][3] else 2) for r in out)
    assert {r["merges"] for r in out} == {1, 2}
    for name in ("t4_mid", "n5_mid"):
        pb, out = runs_of(name)
        counts = [v[1] for r in out for v in r["prune_trace"]]
        assert 0 in counts and 1 in counts and 2 in counts, name
    pb, out = runs_of("n5_alpha0")
    assert all(r["pruned"] == 0 and r["merges"] == pb.n - 1 and r["flags"] == HR.ONE_CLUSTER | HR.NO_SIMILARITY for r in out)
    pb, out = runs_of("n5_alpha1")
    # every merged cluster is cut off at once; the clusters it did not touch keep their pairs and go on merging
    assert all(r["pairs_kept"] == 0 and r["merges"] == pb.n // 2 and r["flags"] == HR.NO_SIMILARITY for r in out)
    pb, out = runs_of("t3_alpha1")   # three nodes: the one other cluster is cut off, nothing is left after one merge
    assert all(r["pairs_kept"] == 0 and r["pruned"] == 1 and r["merges"] == 1 and r["flags"] == HR.NO_SIMILARITY for r in out)
    for name in ("n6_q1", "n6_q2"):
        ev = {}
        pb, S, alpha, runs, seed = HR.run_setup(name)
        for j in range(runs):
            HR.restated_run(pb, S, alpha, seed, j, ev)
        assert ev.get("refused_q", 0) > 0 and ev.get("refused_nan", 0) == 0, name
    ev = {}
    pb, S, alpha, runs, seed = HR.run_setup("bigk")
    for j in range(runs):
        HR.restated_run(pb, S, alpha, seed, j, ev)
    assert ev.get("refused_nan", 0) == 0   # (no edge between 255-state nodes is ever kept on 500 samples: hc_refs.hc_input)
    pb, S, alpha, runs, seed = HR.run_setup("bigk_counts")
    for j in range(runs):
        HR.restated_run(pb, S, alpha, seed, j, ev)
    assert ev.get("refused_nan", 0) > 0
    ev = {}
    pb, S, alpha, runs, seed = HR.run_setup("n33")   # node 32 is tried as a parent and as a child (bit 32 of a ranked mask); it
    for j in range(runs):                             # keeps no edge on these samples, so kept masks past bit 31 are n64's to show
        HR.restated_run(pb, S, alpha, seed, j, ev)
    assert ev.get("refused_q", 0) > 0                 # and here the refusal is at in-degree 3
    pb, out = runs_of("n64")
    assert any(m >> 32 for r in out for m in r["masks"][:32]) and any(m & 0xFFFFFFFF for r in out for m in r["masks"][32:])
    assert all(r["merge_trace"] and max(max(p, c) for p, c, _, _ in r["merge_trace"]) > 64 for r in out)
    pb, out = runs_of("n5_zero")   # 0 / 0: NaN ratios, u < NaN keeps every pair
    assert all(r["pruned"] == 0 and r["merges"] == pb.n - 1 and all(p != p for _, p in r["decisions"]) for r in out)
    pb, out = runs_of("t2_tie")    # alpha = 0 on n = 2: a run is its coin; equal coins give identical runs
    assert len({(HR.bits(r["score"]), tuple(r["masks"])) for r in out}) <= 2


def test_the_clustering_alone_is_the_restated_run_without_its_shuffles():
    """cluster_plan (what the C++ header's host path is held to) against the literal run: with clusters of one node a shuffle
    draws nothing, so as long as a run merges single nodes only the two consume the stream alike -- n = 2 and n = 3 always."""
    for name in ("t2", "t3", "t3_alpha1"):
        pb, S, alpha, runs, seed = HR.run_setup(name)
        for j in range(runs):
            lit = HR.literal_run(pb, S, alpha, seed, j)
            calls, decisions = HR.cluster_plan(S, pb.n, alpha, seed, j)
            assert [(p[0], c[0]) for p, c in calls[:1]] == [(lit["merge_trace"][0][0], lit["merge_trace"][0][1])]
            assert len(calls) == lit["merges"] or pb.n > 2
            assert decisions[:1] == lit["decisions"][:1]


def test_the_package_stream_is_the_library_stream():
    from bayesiannetwork_amd.learning import _Stream
    for seed, j in ((0, 0), (5, 0), (2 ** 63 + 11, 3), (77, 2 ** 33 + 1)):
        a, b = _Stream(seed, j), AR.Stream(seed, j)
        assert [a.next() for _ in range(8)] == [b.next() for _ in range(8)]
        assert [a.below(m) for m in (2, 3, 64)] == [b.below(m) for m in (2, 3, 64)] and a.uniform() == b.uniform()


def _new_row_events():
    out = {}
    for name in HR.NEW_ROWS:
        pb, S, alpha, runs, seed = HR.run_setup(name)
        out[name] = ({}, [])
        for j in range(runs):
            out[name][1].append(HR.restated_run(pb, S, alpha, seed, j, out[name][0]))
    return out


def test_the_new_matrices_are_what_they_say():
    nan_count = inf_count = 0
    for kind in ("sparse_nonfinite", "nan_first", "inf_ties", "inf_sparse"):
        for n in (33, 64):
            S = HR.similarity_matrix(kind, n)
            again = HR.similarity_matrix(kind, n)
            assert np.array_equal(S.view(np.uint64), S.T.copy().view(np.uint64)) and np.array_equal(S.view(np.uint64), again.view(np.uint64))
            upper = S[np.triu_indices(n, 1)]
            share = [np.isnan(upper).mean(), np.isposinf(upper).mean(), np.isneginf(upper).mean()]
            if kind in ("sparse_nonfinite", "nan_first"):
                assert all(0.025 < x < 0.085 for x in share), (kind, n, share)
                assert math.isfinite(S[0][1]) if kind == "sparse_nonfinite" else math.isnan(S[0][1])
            elif kind == "inf_sparse":
                assert share[0] == 0 and share[2] == 0 and 0.025 < share[1] < 0.085
            else:
                at = [HR.list_index(n, x, y) for x, y in HR.INF_TIES_PAIRS]
                assert [i for i, v in enumerate(upper) if v == math.inf] == at                  # (row-major: the list's order)
                assert len({i % 64 for i in at}) == len(at) and all(b - a > 64 for a, b in zip(at, at[1:]))
                assert [i for i, v in enumerate(upper) if v != v] == [HR.list_index(n, *HR.INF_TIES_NAN)] == [1]
            nan_count += int(np.isnan(upper).sum())
            inf_count += int(np.isinf(upper).sum())
    assert nan_count and inf_count


def test_the_new_rows_reach_every_new_event():
    """Together: ties among more than 64 entries, in another lane and in the same lane; NaN at index 0 and elsewhere at a pick;
    p NaN, >= 1 and exactly 0; pruned and kept pairs; visits with 0, 1 and 2 connections; both endings."""
    runs = _new_row_events()
    total = {}
    for events, _ in runs.values():
        for key, count in events.items():
            total[key] = total.get(key, 0) + count
    wanted = ("pick_tie_gt64", "pick_tie_other_lane", "pick_tie_same_lane", "pick_nan_index0", "pick_nan_elsewhere", "p_nan", "p_ge1", "p_zero",
              "pruned", "kept_pair", "visit_0", "visit_1", "visit_2", "refused_q")
    assert all(total.get(key, 0) > 0 for key in wanted), total
    flags = {r["flags"] for _, out in runs.values() for r in out}
    assert HR.NO_SIMILARITY in flags and HR.ONE_CLUSTER | HR.NO_SIMILARITY in flags
    # the rows of finite ties and the one non-finite matrix whose average is not NaN do both: cut and keep, every visit count
    for name in ("n33_ties", "n64_ties", "n33_ties_bound2", "n33_inf_sparse", "n33_inf_sparse_alpha0", "n33_inf_sparse_alpha2"):
        ev = runs[name][0]
        assert all(ev.get(key, 0) > 0 for key in ("pruned", "kept_pair", "visit_0", "visit_1", "visit_2", "pick_tie_other_lane")), (name, ev)
    for name in ("n33_inf_sparse", "n33_inf_sparse_alpha0", "n33_inf_sparse_alpha2"):
        assert all(runs[name][0].get(key, 0) > 0 for key in ("p_nan", "p_ge1", "p_zero")), name
    # a NaN among the initial similarities makes their average NaN: every visit keeps (alpha != 1) or prunes (alpha = 1: pow(1, NaN) = 1)
    for name in ("n33_sparse", "n33_nan_first", "n33_inf_ties", "n33_sparse_alpha0", "n33_sparse_alpha2", "n64_inf_ties"):
        ev, out = runs[name]
        assert ev["p_nan"] == ev["kept_pair"] == ev["visit_2"] and not ev.get("pruned") and all(r["merges"] == len(r["masks"]) - 1 for r in out), name
    ev, out = runs["n33_sparse_alpha1"]
    assert ev["p_ge1"] == ev["pruned"] and not ev.get("kept_pair") and all(r["merges"] == len(r["masks"]) // 2 for r in out)
    assert runs["n33_ties_alpha0"][0]["p_zero"] == runs["n33_ties_alpha0"][0]["kept_pair"] and not runs["n33_ties_alpha0"][0].get("pruned")
    # the first picks the matrices were built for
    first = {name: [r["merge_trace"][0] for r in out] for name, (_, out) in runs.items()}
    assert all(HR.canonical_bits(v) == HR.bits(math.nan) and {p, c} == {0, 1} for p, c, v, _ in first["n33_nan_first"])
    for name in ("n33_inf_ties", "n64_inf_ties"):
        for r in runs[name][1]:
            (p0, c0, v0, _), (p1, c1, v1, _) = r["merge_trace"][:2]
            assert {p0, c0} == set(HR.INF_TIES_PAIRS[0]) and v0 == HR.bits(math.inf)     # the first +inf in list order
            assert {p1, c1} == set(HR.INF_TIES_NAN) and HR.canonical_bits(v1) == HR.bits(math.nan)   # then the NaN, moved to index 0
    assert runs["n33_ties_bound2"][0]["refused_q"] > 0 and all(bin(m).count("1") <= 2 for r in runs["n33_ties_bound2"][1] for m in r["masks"])
    assert any(bin(m).count("1") == 2 for r in runs["n33_ties_bound2"][1] for m in r["masks"])
