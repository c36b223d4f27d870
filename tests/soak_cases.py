"""Deterministic case generators and checks of the randomised parity soaks (tests/test_soak_gpu.py, scripts/soak_*_gpu.py).

Every case is a pure function of (leg, seed, index): its generator is np.random.default_rng([seed, leg id, index]), and every
draw a case may need is made in `*_case`, whether or not the checks use it.  A case can therefore be rebuilt alone, without
drawing the ones before it, and is named `leg:seed:index` (`parse_key` / `make_case`); every assertion message starts with it.

Legs:
- `bp`        random grids, chains and DAGs x evidence x eps: every belief-propagation path against the oracle and against
              each other (what scripts/soak_gpu.py has always compared);
- `samplers`  likelihood weighting, rejection sampling and CPT fitting against the oracle (scripts/soak_samplers_gpu.py);
- `tables`    one random pattern table per case through the five table kernel families -- entropy / all-pairs MI, CPT
              fitting, log-likelihood / AIC / MDL, batched family scores, the subset lattice -- each against the plain host
              reference of tests/*_refs.py under the bound that module states, plus the searches and one cross-check between
              the counting kernel and the all-pairs kernel.

`check_*` take the case and the modules under test (the engine module or the package, and the oracle), make the comparisons and
return a record of what was exercised.  Nothing of the product is imported at module level: the generators need no device."""
import math

import numpy as np

LEGS = {"bp": 0, "samplers": 1, "tables": 2}
# what tests/test_soak_gpu.py runs: the seed, the number of cases (indices 0 .. cases - 1) and the cases per test of each leg
SUITE = {"bp": {"seed": 12345, "cases": 150, "chunk": 10}, "samplers": {"seed": 99, "cases": 40, "chunk": 10},
         "tables": {"seed": 2024, "cases": 48, "chunk": 8}}
LEFT_OUT_SHARE = 0.02   # of the bp cases, at most, may be left out of the sweep comparison

# ---- keys ---------------------------------------------------------------------------------------------

def case_key(leg, seed, index) -> str:
    return f"{leg}:{int(seed)}:{int(index)}"


def parse_key(key):
    leg, seed, index = key.split(":")
    if leg not in LEGS:
        raise ValueError(f"unknown leg {leg!r} (one of {sorted(LEGS)})")
    return leg, int(seed), int(index)


def case_rng(leg, seed, index):
    return np.random.default_rng([int(seed), LEGS[leg], int(index)])


def make_case(leg, seed, index):
    return {"bp": bp_case, "samplers": samplers_case, "tables": tables_case}[leg](seed, index)


def _seed30(r):
    return int(r.integers(1, 1 << 30))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- leg bp ---------------------------------------------------------------------------------------------

FORCE = {0: {"multisweep": 0}, 2: {"multisweep": 2, "small": 0, "mid": 0, "dag": 0}, 3: {"small": 2, "mid": 0, "dag": 0},
         4: {"mid": 2, "small": 0, "dag": 0}, 5: {"dag": 2}}
DEFAULTS = {"multisweep": 1, "small": 1, "mid": 1, "dag": 1, "dagflow": 0}
ELIGIBLE = {2: "resident_eligible", 3: "small_eligible", 4: "mid_eligible", 5: "dag_eligible"}
BATCH_MAX_NODES = 3000
REASSOCIATION_MARGIN = 1e-12   # absolute distance a residual must keep from eps on a path that re-associates


def _bp_network(r):
    from bayesiannetwork_amd import synth
    kind = r.integers(0, 5)
    seed = _seed30(r)
    if kind == 0:
        rows, cols = int(r.integers(2, 90)), int(r.integers(2, 90))
        return f"grid{rows}x{cols}", synth.grid(rows, cols, int(r.choice([2, 3, 4])), seed=seed)
    if kind == 1:
        n = int(r.integers(5, 600))
        return f"chain{n}", synth.random_dag(n, 1, int(r.integers(1, 8)), int(r.choice([2, 3, 4, 5])), seed=seed)
    n = int(r.choice([30, 80, 200, 500, 1200, 3000, 6000]))
    mp = int(r.integers(2, 6))
    arities = [4] if kind == 2 else [int(x) for x in r.choice([2, 3, 4, 5, 6], size=int(r.integers(1, 5)))]
    if kind == 3:
        arities = [int(x) for x in r.choice([2, 3, 4], size=int(r.integers(1, 4)))]
    return (f"dag{n}_p{mp}_k{''.join(map(str, arities))}",
            synth.random_dag(n, mp, int(r.choice([8, 32, 64, 256])), arities if len(arities) > 1 else arities[0], seed=seed))


def bp_case(seed, index):
    """One network, one evidence set, eps and a sweep cap, and the draws of every periodic comparison (shards on every fifth
    index, reload on every seventh, likelihood weighting on every eighth)."""
    from bayesiannetwork_amd import Evidence, synth
    r = case_rng("bp", seed, index)
    name, g = _bp_network(r)
    exact = int(np.diff(g.in_ptr).max()) <= 2 if g.n else True
    # (the tile kernels' any-arity variant keeps the reference's order for tables of up to 128 entries; a two-parent node of arity 6 has 216)
    exact_tiles = exact and int(np.diff(g.cpt_off).max()) <= 128
    ev = synth.random_evidence(g, float(r.choice([0.0, 0.02, 0.1, 0.3])), seed=_seed30(r))
    soft_draw, soft_nodes = r.random(), r.choice(g.n, size=min(g.n, 3), replace=False)
    soft_vals = [0.05 + r.random(int(g.k[v])) for v in soft_nodes]
    if soft_draw < 0.25 and g.n:   # soft evidence on a few nodes: positive weights, not normalised (the reference takes the vector as it is)
        d = {int(v): x for v, x in zip(soft_nodes, soft_vals)}
        hard = {int(v): int(np.argmax(ev.val[ev.off[j]:ev.off[j + 1]])) for j, v in enumerate(ev.node) if int(v) not in d}
        ev = Evidence.from_dict(g, {**hard, **d})
    eps = float(r.choice([1e-3, 1e-6, 1e-9]))
    cap = int(r.choice([0, 0, 0, 3, 40]))
    special, long_cap, v0 = r.random(), int(r.choice([1030, 2060])), int(r.integers(0, g.n))
    beyond_launch = zero_evidence = False
    if special < 0.04 and g.n <= 1200:      # a run beyond one launch's budget of 1 024 iterations (every one-launch path continues from its state in memory)
        eps, cap, beyond_launch = 0.0, long_cap, True
    elif special < 0.08 and g.n:            # an all-zero evidence vector: 0 / 0 -> NaN in the reference (no zero guard); the NaNs must coincide
        hard = {int(v): (ev.val[ev.off[j]:ev.off[j + 1]].copy()) for j, v in enumerate(ev.node)}
        hard[v0] = np.zeros(int(g.k[v0]))
        ev = Evidence.from_dict(g, hard)
        cap, zero_evidence = cap or 12, True
    batch_seeds = (_seed30(r), _seed30(r))
    nranks, owner_draw, overlapped = int(r.integers(2, 6)), r.random(), bool(r.integers(0, 2))
    owner = r.integers(0, nranks, size=g.n).astype(np.int32)
    reload_seed, lw_ev_seed, lw_seed = _seed30(r), _seed30(r), _seed30(r)
    case = {"leg": "bp", "key": case_key("bp", seed, index), "index": int(index), "name": name, "g": g, "ev": ev, "eps": eps, "cap": cap,
            "exact": exact, "exact_tiles": exact_tiles, "beyond_launch": beyond_launch, "zero_evidence": zero_evidence,
            "batch_seeds": batch_seeds if g.n <= BATCH_MAX_NODES else None, "shards": None, "reload_seed": None, "lw": None}
    if index % 5 == 0 and 4 <= g.n <= 4000:   # default stripes, or a random owner map (cuts almost every edge)
        case["shards"] = {"nranks": nranks, "owner": None if owner_draw < 0.6 else owner, "overlapped": overlapped}
    if index % 7 == 0 and g.n <= 6000:
        case["reload_seed"] = reload_seed
    if index % 8 == 0 and g.n <= 6000:
        case["lw"] = (lw_ev_seed, lw_seed)
    return case


def oracle_threads(case) -> int:
    """Host threads for the oracle's sweeps (its loops over the nodes give identical results on any number)."""
    return 1 if case["g"].n < 400 else 16


def bp_oracle(case, oracle, threads=1):
    return oracle.bp_run(case["g"], case["ev"], case["eps"], case["cap"], threads=threads)


def bp_margins(case, want):
    """(a sweep count must be equal on a path that keeps the reference's order, ... on one that re-associates): the oracle's
    residual history stays clear of eps -- helpers.margin_ok, and for re-association also |r - eps| > 1e-12 absolute.  With
    eps = 0 the stopping test `residual < eps` is false for every residual, so the sweep cap decides on every path alike and
    equal counts are required whatever the residuals are."""
    import helpers
    if case["eps"] == 0.0:
        return True, True
    r = np.asarray(want["residuals"], float)
    keeps = helpers.margin_ok(r, case["eps"])
    return keeps, keeps and bool((np.abs(r - case["eps"]) > REASSOCIATION_MARGIN).all())


def bp_left_out_by_oracle(case, want) -> bool:
    """What the oracle alone decides: the case is left out of the sweep comparison on some path it may take."""
    keeps, reassoc = bp_margins(case, want)
    return not keeps or (not case["exact_tiles"] and not reassoc)


def check_bp(case, engine_mod, oracle, threads=None):
    """The comparisons of scripts/soak_gpu.py on one case.  Returns {"paths": forced paths taken (5f: the dataflow form),
    "default": the default path, "batch", "shards": None / "stripes" / "owner map", "reload", "lw", "beyond_launch",
    "zero_evidence", "left_out": a sweep comparison was left out, "comparisons"}."""
    from bayesiannetwork_amd import FlatModel, synth
    from bayesiannetwork_amd.synth import _random_cpts
    Engine = engine_mod.Engine
    key, g, ev, eps, cap = case["key"], case["g"], case["ev"], case["eps"], case["cap"]
    want = bp_oracle(case, oracle, oracle_threads(case) if threads is None else threads)
    keeps, reassoc = bp_margins(case, want)
    rec = {"paths": [], "default": None, "batch": False, "shards": None, "reload": False, "lw": False, "left_out": False,
           "beyond_launch": case["beyond_launch"] and want["sweeps"] > 1024, "zero_evidence": case["zero_evidence"], "comparisons": 0,
           "sweeps": want["sweeps"]}

    def against_oracle(got, exact, what):
        if keeps if exact else reassoc:
            assert got["sweeps"] == want["sweeps"], f"{key}: {case['name']} {what}: {got['sweeps']} sweeps, the oracle {want['sweeps']}"
        else:
            rec["left_out"] = True
            if got["sweeps"] != want["sweeps"]:
                return   # (different sweep counts within the margin: the marginals are those of different sweeps)
        a, b = got["beliefs"], want["beliefs"]
        if exact:
            assert np.array_equal(a, b, equal_nan=True), f"{key}: {case['name']} {what}: marginals are not the oracle's bits"
        else:
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan), f"{key}: {case['name']} {what}: NaNs do not coincide with the oracle's"
            worst = 0.0 if nan.all() else float(np.abs(a[~nan] - b[~nan]).max())
            assert worst < 1e-12, f"{key}: {case['name']} {what}: marginals differ from the oracle's by {worst:.3g}"
        rec["comparisons"] += 1

    def keeps_order(path):   # the item kernels (3, 4) keep the oracle's order for any parent count; the others re-associate beyond two parents
        return (case["exact_tiles"] if path in (0, 2) else case["exact"]) or path in (3, 4)

    with Engine(g) as e:
        def opts(d):
            for k, v in {**DEFAULTS, **d}.items():
                e.set_option(k, v)
        opts({})
        got = e.bp_run(ev, eps, cap)
        rec["default"] = e.last_path()
        against_oracle(got, keeps_order(rec["default"]), f"default path {rec['default']}")
        for path, force in FORCE.items():
            if path in ELIGIBLE and not e.info(ELIGIBLE[path]):
                continue
            opts(force)
            r = e.bp_run(ev, eps, cap)
            if e.last_path() != path:
                continue
            rec["paths"].append(path)
            against_oracle(r, keeps_order(path), f"path {path}")
            if path == 5:
                e.set_option("dagflow", 1)
                f = e.bp_run(ev, eps, cap)
                if e.info("last_dag_flow") == 1:
                    assert f["sweeps"] == r["sweeps"] and np.array_equal(f["beliefs"], r["beliefs"], equal_nan=True), \
                        f"{key}: {case['name']} the DAG path's dataflow form differs from its barrier form"
                    rec["paths"].append("5f")
                    rec["comparisons"] += 1
                e.set_option("dagflow", 0)
        opts({})
        if case["batch_seeds"] is not None:
            sets = [ev, synth.random_evidence(g, 0.05, seed=case["batch_seeds"][0]), synth.random_evidence(g, 0.2, seed=case["batch_seeds"][1])]
            out = e.bp_run_batch(sets, eps, cap)
            batch_path = e.last_path()
            for q, s in enumerate(sets):
                single = e.bp_run(s, eps, cap)
                assert int(out["sweeps"][q]) == single["sweeps"] and np.array_equal(out["beliefs"][q], single["beliefs"], equal_nan=True), \
                    (f"{key}: {case['name']} batch set {q} (batch path {batch_path}, single path {e.last_path()}): sweeps {int(out['sweeps'][q])} / "
                     f"{single['sweeps']}, eps {eps}, cap {cap}")
            rec["batch"] = True
            rec["comparisons"] += 1
    if case["shards"] is not None:   # the multi-GPU data path on ONE device: 2-5 shard engines, emulated all-gather, against the unsharded tile kernels
        sh = case["shards"]
        with Engine(g) as single:
            for k in ("small", "mid", "dag"):
                single.set_option(k, 0)
            ws = single.bp_run(ev, eps, cap)
        shards = [Engine(g, rank=rank, nranks=sh["nranks"], owner=sh["owner"]) for rank in range(sh["nranks"])]
        try:
            out = engine_mod.run_shards_on_one_device(shards, ev, eps, cap, overlapped=sh["overlapped"])
            bel = sum(s.bp_beliefs() for s in shards)
        finally:
            for s in shards:
                s.close()
        rec["shards"] = "stripes" if sh["owner"] is None else "owner map"
        assert out["sweeps"] == ws["sweeps"] and np.array_equal(bel, ws["beliefs"], equal_nan=True), \
            f"{key}: {case['name']} {sh['nranks']} shards ({rec['shards']}) differ from the unsharded run"
        rec["comparisons"] += 1
    if case["reload_seed"] is not None:   # new tables on the same structure: a reloaded engine against a fresh one, on the default path
        _, cpt2 = _random_cpts(g.k, g.in_ptr, g.in_idx, case["reload_seed"])
        g2 = FlatModel(g.k, g.in_ptr, g.in_idx, g.cpt_off, cpt2)
        with Engine(g) as a, Engine(g2) as b:
            a.bp_run(ev, eps, cap)
            a.reload_cpt(g2.cpt)
            ra, rb = a.bp_run(ev, eps, cap), b.bp_run(ev, eps, cap)
            assert a.last_path() == b.last_path() and ra["sweeps"] == rb["sweeps"] and np.array_equal(ra["beliefs"], rb["beliefs"], equal_nan=True), \
                f"{key}: {case['name']} a reloaded engine differs from a fresh one"
        rec["reload"] = True
        rec["comparisons"] += 1
    if case["lw"] is not None:   # likelihood weighting on the same network: the weighted histogram of 2 048 samples against the oracle's
        st = synth.random_evidence(g, 0.05, seed=case["lw"][0]).hard_states(g)
        with Engine(g) as e:
            h = e.lw_run(st, 2048, seed=case["lw"][1])
        o = oracle.lw_run(g, st, 2048, seed=case["lw"][1])
        assert np.allclose(h, o["hist"], rtol=1e-9, atol=1e-12), \
            f"{key}: {case['name']} likelihood weighting differs from the oracle by {float(np.abs(h - o['hist']).max()):.3g}"
        rec["lw"] = True
        rec["comparisons"] += 1
    return rec


def bp_line(case, rec) -> str:
    return (f"{case['key']:14s} {case['name']:28s} n={case['g'].n:5d} eps={case['eps']:g} cap={case['cap']:4d} sweeps={rec['sweeps']:4d} "
            f"default={rec['default']} forced={rec['paths']}" + (" left out of the sweep comparison" if rec["left_out"] else ""))


# ---- leg samplers ---------------------------------------------------------------------------------------

def samplers_case(seed, index):
    from bayesiannetwork_amd import synth
    r = case_rng("samplers", seed, index)
    n = int(r.choice([8, 40, 150, 600, 2500, 9000]))
    mp = int(r.integers(1, 7))
    if r.random() < 0.4:
        arities = [int(x) for x in r.choice([2, 3, 4], size=int(r.integers(1, 4)))]     # the straight-line kernel's domain (if tables <= 256 rows, <= 4 parents)
    else:
        arities = [int(x) for x in r.choice([1, 2, 3, 4, 5, 7, 8], size=int(r.integers(1, 4)))]
    g = synth.random_dag(n, mp, int(r.choice([4, 16, 64])), arities if len(arities) > 1 else arities[0], seed=_seed30(r))
    st = synth.random_evidence(g, float(r.choice([0.0, 0.03, 0.15])), seed=_seed30(r)).hard_states(g)
    ns_small, ns_large = int(r.choice([64, 1000, 4096, 20000])), int(r.choice([64, 1000]))
    lw_seed, begin, accept = int(r.integers(1, 1 << 40)), int(r.choice([0, 7, 1 << 33])), int(r.choice([10, 200]))
    return {"leg": "samplers", "key": case_key("samplers", seed, index), "index": int(index), "g": g, "n": n, "max_parents": mp, "arities": arities,
            "st": st, "ns": ns_small if n <= 2500 else ns_large, "seed": lw_seed, "begin": begin, "accept": accept}


def check_samplers(case, engine_mod, oracle):
    """States bit-equal to the oracle's, weights <= 1e-12 relative, the weighted histogram <= 1e-9 (fp64 atomics order);
    rejection sampling: counts, draws and acceptances exact; CPT fitting from the sampled patterns bit-equal to the restatement."""
    key, g, st, ns, seed, begin = case["key"], case["g"], case["st"], case["ns"], case["seed"], case["begin"]
    rec = {"kernel": None, "rs": False, "fit": False, "comparisons": 0}
    with engine_mod.Engine(g) as e:
        hist = e.lw_run(st, ns, seed=seed, sample_begin=begin)
        small = e.info("lw_small")
        rec["kernel"] = "straight-line" if small else "generic"
        states, weights = e.lw_states(ns)
        o = oracle.lw_run(g, st, ns, seed=seed, s_begin=begin, states_cap=ns)
        assert np.array_equal(states, o["states"]), f"{key}: {g.name} states ({rec['kernel']} kernel)"
        assert np.allclose(weights, o["weights"], rtol=1e-12, atol=0), f"{key}: {g.name} weights"
        assert np.allclose(hist, o["hist"], rtol=1e-9, atol=1e-12), f"{key}: {g.name} histogram"
        rec["comparisons"] += 3
        if case["n"] <= 600:
            c, drawn, acc = e.rs_run(st, case["accept"], seed=seed, max_draw=1 << 16, sample_begin=begin)
            wc, wd, wa = oracle.rs_run(g, st, case["accept"], seed=seed, s_begin=begin, max_draw=1 << 16)
            assert (drawn, acc) == (wd, wa) and np.array_equal(c, wc), f"{key}: {g.name} rejection sampling: drawn {drawn} / {wd}, accepted {acc} / {wa}"
            rec["rs"] = True
            rec["comparisons"] += 1
        if case["n"] <= 150 and ns >= 1000:
            pats, cnts = np.unique(states, axis=0, return_counts=True)
            assert np.array_equal(e.fit_cpt(pats, cnts), oracle.make_cpt(g, pats, cnts)), f"{key}: {g.name} fit_cpt"
            rec["fit"] = True
            rec["comparisons"] += 1
    return rec


def samplers_line(case, rec) -> str:
    return (f"{case['key']:18s} {case['g'].name:28s} n={case['n']:5d} max parents={case['max_parents']} arities={case['arities']} "
            f"samples={case['ns']} kernel={rec['kernel']}")


# ---- leg tables -----------------------------------------------------------------------------------------

MAX_PARENTS, MAX_ENTRIES, MAX_LATTICE_CELLS = 16, 1 << 20, 1 << 25
LDS_CELLS = 4096                                     # counters in LDS up to this many cells (CPT fitting, family counting, the lattice's one-launch form)
CHUNK_LDS_CANDIDATES, CHUNK_GLOBAL_CANDIDATES = 32, 8   # candidates one counting chunk takes
MODEL_ENTRIES = 1 << 19                              # all CPTs of a case's structure together (keeps the host references in seconds)
PAIR_STATES = 520                                    # one-hot width of the columns the all-pairs reference takes
FAMILY_WORK, LATTICE_WORK = 60_000, 2_000_000        # patterns x families the host references count per case
WEIGHTS = [1, 127, 128, (1 << 31) - 1, 1 << 31, 1 << 40]
EDGE_ARITIES = ([1, 2, 3, 4, 5], [16, 17, 32, 33], [241, 255])
SEARCH_COLUMNS = 12


def _tables_arities(r, n):
    kind = r.choice(4, size=n, p=[0.62, 0.2, 0.08, 0.10])
    k = np.zeros(n, np.int64)
    for i in range(n):
        k[i] = int(r.integers(6, 256)) if kind[i] == 3 else int(r.choice(EDGE_ARITIES[kind[i]]))
    if r.random() < 0.4:   # the fixed share with an arity-1 column, half of the time the column with the smallest id
        k[0 if r.random() < 0.5 else int(r.integers(0, n))] = 1
    return k


def _pattern_count(r) -> int:
    u = r.random()
    if u < 0.08:
        return 1
    if u < 0.6:
        base, top = [(8, 40), (64, 20), (256, 8), (2048, 4), (4096, 2)][int(r.integers(0, 5))]
        return base * int(r.integers(1, top + 1)) + int(r.integers(-1, 2))
    return int(r.integers(2, 10_001))


def _pick(r, pool):
    return int(pool[int(r.integers(0, len(pool)))])


def _grow(r, k, pool, want, cells, fits):
    """Up to `want` columns drawn one at a time from those of `pool` that still fit: fits(cells with the column, column)."""
    out, pool = [], list(pool)
    while len(out) < want:
        ok = [u for u in pool if fits(cells * int(k[u]), u)]
        if not ok:
            break
        u = _pick(r, ok)
        out.append(u)
        pool.remove(u)
        cells *= int(k[u])
    return out, cells


def _grow_lattice(r, k, pool, want, cells, all_cells):
    """Up to `want` lattice candidates, one at a time from the columns that keep the top family within 2^20 entries (`cells` so
    far) and the 2^m tables together within 2^25 cells (`all_cells` so far)."""
    out, pool = [], list(pool)
    while len(out) < want:
        got, cells = _grow(r, k, pool, 1, cells, lambda c, u: c <= MAX_ENTRIES and all_cells * (int(k[u]) + 1) <= MAX_LATTICE_CELLS)
        if not got:
            break
        out += got
        pool.remove(got[0])
        all_cells *= int(k[got[0]]) + 1
    return out


def _parent_count(r) -> int:
    return int(r.choice([0, 1, 2, 3, 4, int(r.integers(5, MAX_PARENTS + 1))], p=[0.25, 0.25, 0.2, 0.12, 0.08, 0.1]))


def tables_case(seed, index):
    """One pattern table (columns, patterns, weights), a DAG over its columns, groups and lattices of candidate families,
    variable lists, pairs and -- up to SEARCH_COLUMNS columns -- searches.  Every limit of the library's input domain is
    respected while drawing: a column is drawn from those that still fit."""
    r = case_rng("tables", seed, index)
    n = int(r.integers(3, SEARCH_COLUMNS + 1)) if r.random() < 0.45 else int(r.integers(SEARCH_COLUMNS + 1, 41))
    k = _tables_arities(r, n)
    P = _pattern_count(r)
    pats = np.stack([r.integers(0, kk, P) for kk in k], axis=1).astype(np.uint8)
    if P > 1 and r.random() < 0.5:   # duplicate rows
        dst, src = r.integers(0, P, size=max(1, P // 4)), r.integers(0, P, size=max(1, P // 4))
        pats[dst] = pats[src]
    mode = int(r.integers(0, 4))
    w = r.choice(np.array([[1], [1, 127, 128], WEIGHTS, WEIGHTS][mode], np.uint64), P)
    zero_draw, zeros, keep = r.random(), r.random(P) < 0.2, int(r.integers(0, P))
    if zero_draw < 0.4:
        w[zeros] = 0
        if not w.any():
            w[keep] = 1
    total = int(w.astype(object).sum())
    assert 0 < total < 1 << 64

    # the structure: nodes in a random order, each drawing its parents among the earlier ones that fit
    order, parents, used = r.permutation(n), [[] for _ in range(n)], 0
    for i, v in enumerate(int(x) for x in order):
        room = min(MAX_ENTRIES, MODEL_ENTRIES - used - 255 * (n - 1 - i))
        ps, cells = _grow(r, k, [int(u) for u in order[:i]], _parent_count(r), int(k[v]), lambda c, u: c <= room)
        parents[v], used = sorted(ps), used + cells

    # groups of candidate families: (child, base increasing, candidates in any order)
    family_room = max(3, FAMILY_WORK // P)
    groups, many = [], r.random() < 0.2
    for gi in range(int(r.integers(1, 5))):
        child = int(r.integers(0, n))
        others = [u for u in range(n) if u != child]
        base, cells = _grow(r, k, others, int(r.choice([0, 1, 2, 3, int(r.integers(4, 9))], p=[0.2, 0.3, 0.25, 0.15, 0.1])), int(k[child]),
                            lambda c, u: c <= MAX_ENTRIES)
        want = min(family_room, len(others)) if many and gi == 0 else min(family_room, int(r.integers(0, 13)))
        cand = []   # each candidate is one more parent of the BASE: base + u within the limits, whatever the other candidates are
        pool = [u for u in others if u not in base and cells * int(k[u]) <= MAX_ENTRIES]
        for _ in range(min(want, len(pool))):
            cand.append(pool.pop(int(r.integers(0, len(pool)))))
        family_room = max(0, family_room - 1 - len(cand))
        groups.append((child, sorted(base), cand))
        if family_room == 0:
            break
    # the same families grouped differently: a family is the base of a group or the candidate of the base without one of its parents
    regroup = {}
    fams = [(c, tuple(sorted(b))) for c, b, _ in groups] + [(c, tuple(sorted(b + [u]))) for c, b, us in groups for u in us]
    for j in r.permutation(len(fams)):
        c, ps = fams[int(j)]
        if ps and r.random() < 0.6:
            u = _pick(r, ps)
            slot = regroup.setdefault((c, tuple(x for x in ps if x != u)), [False, []])
            if u not in slot[1]:
                slot[1].append(u)
        else:
            regroup.setdefault((c, ps), [False, []])[0] = True
    regroup = [(c, list(b), us) for (c, b), (_, us) in regroup.items()]

    # lattices: (child, base in any order, candidates in any order); the top family and the 2^m tables within the limits
    m_room = min(12, max(0, int(math.log2(max(1, LATTICE_WORK // P)))))
    lattices = []
    for _ in range(int(r.integers(1, 3))):
        child = int(r.integers(0, n))
        others = [u for u in range(n) if u != child]
        base, cells = _grow(r, k, others, int(r.choice([0, 1, 2, int(r.integers(3, 9))], p=[0.35, 0.3, 0.2, 0.15])), int(k[child]),
                            lambda c, u: c <= MAX_ENTRIES)
        want = min(int(r.integers(0, 13)), m_room, MAX_PARENTS - len(base))
        cand = _grow_lattice(r, k, [u for u in others if u not in base], want, cells, cells)
        lattices.append((child, base, cand))

    var_lists = [[int(x) for x in r.integers(0, n, size=int(r.integers(1, 6)))] for _ in range(3)]
    # the columns of the all-pairs comparison: every column while the one-hot width allows, else a run of a random order
    pair_cols, width = [], 0
    for u in (int(x) for x in r.permutation(n)):
        if width + int(k[u]) <= PAIR_STATES or len(pair_cols) < 2:
            pair_cols.append(u)
            width += int(k[u])
    if len(pair_cols) == n:
        pair_cols = list(range(n))
    cross = []
    for _ in range(3):
        c, u = (int(x) for x in r.choice(pair_cols, size=2, replace=False))
        cross.append((c, u))
    node_selection = [int(x) for x in r.permutation(n)[:int(r.integers(1, n + 1))]]

    case = {"leg": "tables", "key": case_key("tables", seed, index), "index": int(index), "k": k.astype(np.int32), "pats": pats, "counts": w,
            "total": total, "parents": parents, "groups": groups, "regroup": regroup, "lattices": lattices, "var_lists": var_lists,
            "pair_cols": pair_cols, "cross": cross, "node_selection": node_selection, "split_for_lattice": int(r.choice([1, 2, 7])),
            "search": None}
    criterion, max_parents = ("aic", "mdl")[int(r.integers(0, 2))], int(r.choice([MAX_PARENTS, 2, 3]))
    scans = [(int(r.integers(0, n)), [int(x) for x in r.permutation(n)] + [int(r.integers(0, n))]) for _ in range(3)]
    best, best_children = [], [int(x) for x in r.permutation(n)[:2]]   # (distinct children: each starts without parents)
    for child in best_children:
        cand = _grow_lattice(r, k, [u for u in range(n) if u != child], 6, int(k[child]), int(k[child]))
        best.append((child, cand + cand[:1] + [child]))   # (a candidate twice and the child itself: both are passed over)
    vs, pool = [], [int(x) for x in r.permutation(n)]
    for u in pool:   # brute force: every vertex's lattice over the others within the limits
        trial = vs + [u]
        top = math.prod(int(k[x]) for x in trial)
        if len(vs) < 4 and top <= MAX_ENTRIES and all(int(k[v]) * math.prod(int(k[x]) + 1 for x in trial if x != v) <= MAX_LATTICE_CELLS for v in trial):
            vs = trial
    if n <= SEARCH_COLUMNS:
        case["search"] = {"criterion": criterion, "max_parents": max_parents, "scans": scans, "best": best, "brute": vs}
    return case


def families_of(groups):
    for c, b, us in groups:
        yield c, tuple(sorted(b))
        for u in us:
            yield c, tuple(sorted(list(b) + [u]))


def subset(cand, mask):
    return [cand[j] for j in range(len(cand)) if (mask >> j) & 1]


def group_chunks(k, group) -> int:
    """How many counting chunks one group takes (bn_learn.hpp: families of <= 4 096 cells share LDS blocks of 4 096 cells, at
    most 32 candidates each; larger ones are counted in device memory, at most 8 candidates per chunk)."""
    c, b, us = group
    base = int(k[c]) * math.prod(int(k[u]) for u in b)
    chunks = 0
    for lds in (True, False):
        open_, n_cand, cells = False, 0, 0
        for j, fam in enumerate([base] + [base * int(k[u]) for u in us]):
            if (fam <= LDS_CELLS) != lds:
                continue
            if not open_ or n_cand >= (CHUNK_LDS_CANDIDATES if lds else CHUNK_GLOBAL_CANDIDATES) or (lds and cells + fam > LDS_CELLS):
                chunks, open_, n_cand, cells = chunks + 1, True, 0, 0
            n_cand += j > 0   # (the base takes no candidate slot)
            cells += fam
    return chunks


def tables_domain_ok(case):
    """The library's input domain, from the case alone: <= 16 parents, family tables <= 2^20 entries, lattice scratch <= 2^25
    cells, total weight in 1 .. 2^64 - 1, states below the arities."""
    k = [int(x) for x in case["k"]]

    def cells(child, ps):
        return k[child] * math.prod(k[u] for u in ps)
    ok = 0 < case["total"] < 1 << 64 and bool((case["pats"] < case["k"][None, :]).all())
    for v, ps in enumerate(case["parents"]):
        ok &= len(ps) <= MAX_PARENTS and cells(v, ps) <= MAX_ENTRIES and ps == sorted(set(ps)) and v not in ps
    for groups in (case["groups"], case["regroup"]):
        for c, ps in families_of(groups):
            ok &= len(ps) <= MAX_PARENTS and len(set(ps)) == len(ps) and c not in ps and cells(c, ps) <= MAX_ENTRIES
    lattices = list(case["lattices"])
    if case["search"]:
        lattices += [(c, [], sorted(set(cand) - {c})) for c, cand in case["search"]["best"]]
        lattices += [(v, [], [u for u in case["search"]["brute"] if u != v]) for v in case["search"]["brute"]]
    for c, b, cand in lattices:
        ok &= len(b) + len(cand) <= MAX_PARENTS and len(set(b + cand)) == len(b + cand) and c not in b + cand
        ok &= cells(c, b + cand) <= MAX_ENTRIES and cells(c, b) * math.prod(k[u] + 1 for u in cand) <= MAX_LATTICE_CELLS
    return bool(ok)


def tables_model(case):
    """The case's structure as a FlatModel with an all-zero CPT (host only)."""
    from bayesiannetwork_amd.learning import _csr, structure_model
    return structure_model(case["k"], *_csr(case["parents"]), name=case["key"])


def tables_forms(case) -> set:
    """The kernel forms a case takes, from its sizes (the thresholds are the headers')."""
    k = [int(x) for x in case["k"]]
    forms = set()
    sizes = [k[c] * math.prod(k[u] for u in ps) for c, ps in families_of(case["groups"])]
    sizes += [k[v] * math.prod(k[u] for u in ps) for v, ps in enumerate(case["parents"])]
    forms |= {"count_lds" if s <= LDS_CELLS else "count_global" for s in sizes}
    for c, b, cand in case["lattices"]:
        forms.add("lattice_lds" if k[c] * math.prod(k[u] for u in b + cand) <= LDS_CELLS else "lattice_levels")
        if cand and k[min(b + cand)] == 1 and min(b + cand) in cand:
            forms.add("lattice_arity1_top_digit")
    if any(group_chunks(k, g) > 1 for g in case["groups"]):
        forms.add("multi_chunk")
    fams = list(families_of(case["groups"])) + [(c, tuple(b + cand)) for c, b, cand in case["lattices"]]
    if 1 in k:   # (every column is a child in the structure the CPTs are fitted to)
        forms.add("arity1_child")
    if any(k[u] == 1 for _, ps in fams for u in ps) or any(k[u] == 1 for ps in case["parents"] for u in ps):
        forms.add("arity1_parent")
    if max(int(x) for x in case["counts"]).bit_length() > 7:
        forms.add("digit_passes>1")
    if (case["counts"] == 0).any():
        forms.add("zero_weights")
    if case["search"]:
        forms.add("search")
    return forms


def check_tables_host(case):
    """The host references against each other on one case, without a device: the lattice's index arithmetic gives direct
    counting's tables, the fitted CPT's node sums are the family terms, pair counts are cell counts."""
    import learning_refs as LR
    import loglik_refs as R
    import pattern_refs as PR
    import subset_refs as SR
    key, k, pats, w = case["key"], case["k"], case["pats"], case["counts"]
    for child, base, cand in case["lattices"]:
        if len(cand) > 6:
            continue
        top = LR.family_counts(pats, w, k, child, base + cand)
        for mask, N in enumerate(SR.lattice_counts(top, k, child, base, cand)):
            assert np.array_equal(N, LR.family_counts(pats, w, k, child, base + subset(cand, mask))), f"{key}: lattice_counts {child} {base} {cand} mask {mask}"
    model = tables_model(case)
    model.cpt[:] = PR.fit_cpt_ref(model, pats, w)
    N = R.family_counts_ref(model, pats, w)
    assert int(N.astype(object).sum()) == case["total"] * model.n, f"{key}: family_counts_ref loses samples"
    ll = R.nodes_ref(model, N)
    table = LR.Table(pats, w, k)
    for v in range(min(model.n, 4)):
        assert ll[v] == table.libm_ll(v, case["parents"][v]), f"{key}: nodes_ref of the fitted model is not the family term of node {v}"
    cols = case["pair_cols"]
    M = PR.pair_count_matrix(pats[:, cols], w, k[cols])
    for i, j in ((0, len(cols) - 1), (len(cols) // 2, 0)):
        cells = sorted(int(x) for x in PR.block(M, k[cols], i, j).ravel() if x)
        assert cells == sorted(PR.cell_counts(pats, w, [cols[i], cols[j]])), f"{key}: pair_count_matrix block {cols[i]}, {cols[j]}"


def check_tables(case, bn, oracle=None):
    """Every table kernel family on one case against its host reference.  `bn`: the bayesiannetwork_amd package.  Returns
    {"forms": kernel forms taken, "digit_passes", "comparisons"}."""
    import learning_refs as LR
    import loglik_refs as R
    import pattern_refs as PR
    import subset_refs as SR
    from bayesiannetwork_amd.engine import Engine, fit_cpt
    from bayesiannetwork_amd.evaluation import AIC, MDL, InfoTable, log_likelihood_nodes, log_likelihood_rows
    from bayesiannetwork_amd.learning import Learner, score_groups, score_subsets
    key, k, pats, w, total = case["key"], case["k"], case["pats"], case["counts"], case["total"]
    n = len(k)
    rec = {"forms": tables_forms(case), "comparisons": 0}

    def done(count=1):
        rec["comparisons"] += count

    with InfoTable(pats, w, k, device=0) as t:
        rec["digit_passes"] = t.info("digit_passes")
        assert (rec["digit_passes"] > 1) == ("digit_passes>1" in rec["forms"]), f"{key}: digit_passes {rec['digit_passes']}"

        # ---- all-pairs counts and entropies, entropy of variable lists ----
        cols = case["pair_cols"]
        kc = k[cols]
        M = PR.pair_count_matrix(pats[:, cols], w, kc)
        pairs = [(x, y) for x in cols for y in cols]
        for (x, y), blk in zip(pairs, t.pair_counts(pairs)):
            assert np.array_equal(blk, PR.block(M, kc, cols.index(x), cols.index(y))), f"{key}: pair_counts of columns {x}, {y}"
        done()
        out = t.pair_entropies(None if cols == list(range(n)) else cols)
        h, hxy, mi = out["h"], out["hxy"], out["mi"]
        ref, nnz = PR.pair_entropies_ref(M, kc, total)
        bad = np.argwhere(~(np.abs(hxy - ref) <= PR.entropy_bound(ref, nnz)))
        assert bad.size == 0, f"{key}: pair_entropies beyond entropy_bound: " + str([(cols[x], cols[y], hxy[x, y], ref[x, y]) for x, y in bad[:5]])
        assert np.array_equal(bits(hxy), bits(hxy.T)), f"{key}: hxy is not symmetric bit for bit"
        assert np.array_equal(bits(np.diag(hxy)), bits(h)), f"{key}: diag(hxy) is not h"
        assert np.array_equal(bits(h[:, None] + h[None, :] - hxy), bits(mi)), f"{key}: mi is not h[x] + h[y] - hxy"
        done(4)
        for vs in case["var_lists"]:
            cells = PR.cell_counts(pats, w, vs)
            exact = PR.entropy_exact(cells)
            got = t.entropy(vs)
            assert abs(got - exact) <= PR.entropy_bound(exact, len(cells)), f"{key}: entropy({vs}) = {got!r}, exact {exact!r}"
            done()

        # ---- CPT fit, log-likelihood rows and nodes, AIC / MDL on the fitted model ----
        model = tables_model(case)
        model.cpt[:] = fit_cpt(model, pats, w, device=0)
        assert np.array_equal(bits(model.cpt), bits(PR.fit_cpt_ref(model, pats, w))), f"{key}: fit_cpt is not fit_cpt_ref"
        done()
        L = R.log_table(model)
        with Engine(model, device=0) as eng:
            for nodes in (None, case["node_selection"]):
                assert np.array_equal(bits(log_likelihood_rows(eng, t, nodes)), bits(R.rows_ref(model, pats, nodes, L))), \
                    f"{key}: log_likelihood_rows, nodes {nodes}"
                done()
            ll_node, N = log_likelihood_nodes(eng, t, counts=True)
            assert np.array_equal(N, R.family_counts_ref(model, pats, w)), f"{key}: log_likelihood_nodes counts"
            assert np.array_equal(bits(ll_node), bits(R.nodes_ref(model, N, L))), f"{key}: log_likelihood_nodes is not nodes_ref"
            done(2)
            seen = w != 0
            table = R.table_dict(pats[seen], w[seen])   # (a sampler's table holds no pattern of count 0)
            bound = R.likelihood_bound(model, N, L)
            for functor, reference in ((AIC, R.reference_aic), (MDL, R.reference_mdl)):
                got, want = functor(t)(eng), reference(model, table)
                assert abs(got - want) <= bound, f"{key}: {functor.__name__} {got!r}, reference {want!r}, bound {bound:.3g}"
                done()

        # ---- batched family scores ----
        groups = case["groups"]
        ll, counts = score_groups(t, groups, counts=True)
        flat_ll = [x for row in ll for x in row]
        by_family, host_counts = {}, {}
        for (c, ps), got_ll, got_N in zip(families_of(groups), flat_ll, [x for row in counts for x in row]):
            want = LR.family_counts(pats, w, k, c, ps)
            assert np.array_equal(got_N, want), f"{key}: score_groups counts of {c} | {list(ps)}"
            exact, bound = math.fsum(LR.family_terms(want, k[c]).tolist()), LR.ll_bound(want, k[c])
            assert abs(got_ll - exact) <= bound, f"{key}: score_groups ll of {c} | {list(ps)}: {got_ll!r}, fsum {exact!r}, bound {bound:.3g}"
            assert by_family.setdefault((c, ps), got_ll) == got_ll, f"{key}: the family {c} | {list(ps)} has two values in one batch"
            host_counts[(c, ps)] = want
            done(2)
        for splits in (1, 2, 7):
            ll_s, counts_s = score_groups(t, groups, counts=True, splits=splits)
            assert np.array_equal(bits([x for row in ll_s for x in row]), bits(flat_ll)), f"{key}: score_groups ll under splits={splits}"
            assert all(np.array_equal(a, b) for ra, rb in zip(counts_s, counts) for a, b in zip(ra, rb)), f"{key}: score_groups counts under splits={splits}"
            done()
        for (c, ps), x in zip(families_of(case["regroup"]), [x for row in score_groups(t, case["regroup"]) for x in row]):
            if (c, ps) in by_family:   # (a regrouped base that was no family of the groups is scored and not compared)
                assert bits([x])[0] == bits([by_family[(c, ps)]])[0], f"{key}: the family {c} | {list(ps)} regrouped has other bits"
        done()

        # ---- the subset lattice ----
        for child, base, cand in case["lattices"]:
            ll_l, N_l = score_subsets(t, child, base, cand, counts=True)
            fams = [(child, sorted(base + subset(cand, mask)), []) for mask in range(1 << len(cand))]
            for mask in range(1 << len(cand)):
                assert np.array_equal(N_l[mask], LR.family_counts(pats, w, k, child, fams[mask][1])), f"{key}: score_subsets counts {child} {base} {cand} mask {mask}"
            batched = [x[0] for x in score_groups(t, fams)]
            assert np.array_equal(bits(batched), bits(ll_l)), f"{key}: score_subsets ll {child} {base} {cand} is not score_groups'"
            ll_s, N_s = score_subsets(t, child, base, cand, counts=True, splits=case["split_for_lattice"])
            assert np.array_equal(bits(ll_s), bits(ll_l)) and all(np.array_equal(a, b) for a, b in zip(N_s, N_l)), \
                f"{key}: score_subsets {child} {base} {cand} under splits={case['split_for_lattice']}"
            done(3)

        # ---- the counting kernel against the all-pairs kernel: ll(c | u) - ll(c | nothing) = N MI(c, u), in bits ----
        for c, u in case["cross"]:
            (ll0, ll1), = score_groups(t, [(c, [], [u])])
            i, j = cols.index(c), cols.index(u)
            N0, N1 = LR.family_counts(pats, w, k, c, []), LR.family_counts(pats, w, k, c, [u])
            bound = (LR.ll_bound(N0, k[c]) + LR.ll_bound(N1, k[c])) / math.log(2.0) + float(total) * (
                PR.entropy_bound(ref[i, i], nnz[i, i]) + PR.entropy_bound(ref[j, j], nnz[j, j]) + PR.entropy_bound(ref[i, j], nnz[i, j]))
            lhs, rhs = (ll1 - ll0) / math.log(2.0), float(total) * mi[i, j]
            assert abs(lhs - rhs) <= bound, f"{key}: ll({c} | {u}) - ll({c}) = {lhs!r} bits, N MI = {rhs!r}, bound {bound:.3g}"
            done()

        # ---- the searches over the device's own terms ----
        if case["search"]:
            s, cache = case["search"], {}

            def terms(child, parents):
                fam = (int(child), tuple(sorted(int(u) for u in parents)))
                if fam not in cache:
                    cache[fam] = score_groups(t, [(fam[0], list(fam[1]), [])])[0][0]
                return cache[fam]

            def same(Lr, ref_, what):
                lls, params = Lr.terms()
                assert Lr.parents() == ref_.parents, f"{key}: {what}: parents {Lr.parents()}, the restatement {ref_.parents}"
                assert bits([Lr.score()])[0] == bits([ref_.score])[0] and np.array_equal(bits(lls), bits(ref_.ll)) and params == ref_.params, \
                    f"{key}: {what}: score {Lr.score()!r}, the restatement {ref_.score!r}"
                done()
            empty = LR.empty_graph(n)
            with Learner(t, None, s["criterion"], s["max_parents"]) as Lr:
                ref_ = LR.RefLearner(k, empty, s["criterion"], total, terms, s["max_parents"])
                for child, cand in s["scans"]:
                    assert Lr.try_parents(child, cand).tolist() == ref_.try_parents(child, cand), f"{key}: try_parents({child}, {cand})"
                    same(Lr, SR.RefSearch(k, ref_.parents, s["criterion"], total, terms, s["max_parents"]), f"try_parents({child}, {cand})")
            with Learner(t, None, s["criterion"], s["max_parents"]) as Lr:
                ref_ = SR.RefSearch(k, empty, s["criterion"], total, terms, s["max_parents"])
                for child, cand in s["best"]:
                    assert Lr.best_parents(child, cand).tolist() == ref_.best_parents(child, cand), f"{key}: best_parents({child}, {cand})"
                    same(Lr, ref_, f"best_parents({child}, {cand})")
            with Learner(t, None, s["criterion"], s["max_parents"]) as Lr:
                ref_ = SR.RefSearch(k, empty, s["criterion"], total, terms, s["max_parents"])
                got, want = Lr.brute_force(s["brute"]), ref_.brute_force(s["brute"])
                assert bits([got])[0] == bits([want])[0], f"{key}: brute_force({s['brute']}) = {got!r}, the restatement {want!r}"
                same(Lr, ref_, f"brute_force({s['brute']})")
    return rec


def tables_line(case, rec) -> str:
    return (f"{case['key']:16s} n={len(case['k']):2d} P={len(case['counts']):5d} groups={len(case['groups'])} "
            f"lattices={[len(c) for _, _, c in case['lattices']]} digits={rec['digit_passes']} forms={sorted(rec['forms'])}")


def suite_chunks(leg):
    """[(first index, one past the last)] of the tests of one leg."""
    cases, chunk = SUITE[leg]["cases"], SUITE[leg]["chunk"]
    return [(a, min(a + chunk, cases)) for a in range(0, cases, chunk)]


CHECKS = {"bp": check_bp, "samplers": check_samplers, "tables": check_tables}
LINES = {"bp": bp_line, "samplers": samplers_line, "tables": tables_line}


# ---- the front end of scripts/soak_*_gpu.py ----------------------------------------------------------------

def modules_for(leg):
    import bayesiannetwork_amd
    import oracle
    from bayesiannetwork_amd import engine
    return (bayesiannetwork_amd,) if leg == "tables" else (engine, oracle)


def run_case(key):
    """Rebuilds the case `leg:seed:index` and runs its check: what the test that names this key runs."""
    leg, seed, index = parse_key(key)
    case = make_case(leg, seed, index)
    rec = CHECKS[leg](case, *modules_for(leg))
    print(f"{LINES[leg](case, rec)}  [{rec['comparisons']} comparisons]", flush=True)
    return rec


def soak_main(argv, legs, default_leg, default_seed):
    """[seconds] [seed] [--leg LEG]: cases 0, 1, ... of (leg, seed) until the budget is spent; --case leg:seed:index: that one
    case.  Stops at the first difference with the case's key in the message."""
    import time
    args = list(argv)
    if "--case" in args:
        run_case(args[args.index("--case") + 1])
        return 0
    leg = default_leg
    if "--leg" in args:
        at = args.index("--leg")
        leg = args[at + 1]
        del args[at:at + 2]
        if leg not in legs:
            raise SystemExit(f"--leg: one of {legs}")
    budget = float(args[0]) if args else 240.0
    seed = int(args[1]) if len(args) > 1 else default_seed
    t_end, count, comparisons = time.time() + budget, 0, 0
    while time.time() < t_end:
        comparisons += run_case(case_key(leg, seed, count))["comparisons"]
        count += 1
    print(f"soak ok: leg {leg}, seed {seed}: {count} cases, {comparisons} comparisons")
    return 0
