"""The fixtures tests/golden/learn_*.npz: what the reference's OWN sampler::make_cpt, aic / mdl, greedy, k2_algorithm, brute_force
and stepwise_structure did (oracle/ref_learn_driver.cpp over the unmodified headers) on this project's fixed inputs, and the
reading of its evaluation logs.  `run_specs` says which commands a fixture holds (tests/golden/make_golden.py --learning runs
them), `load` reads a fixture back, the rest turns a log -- every graph the reference's Eval was asked about, in order, with the
double it returned -- into the decisions the reference took, using nothing but the logged graphs themselves."""
import os

import numpy as np

import learning_refs as LR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRY_KINDS = ("greedy_all", "greedy_vertexes", "greedy_hint", "k2")
BRUTE_KINDS = ("brute_all", "brute_vertexes", "brute_hint")


def fixture_names():
    return sorted(f[len("learn_"):-len(".npz")] for f in os.listdir(GOLDEN) if f.startswith("learn_") and f.endswith(".npz"))


# ---- which commands a fixture holds ------------------------------------------------------------------------

def input_table(name) -> LR.Table:
    if name in ("n5", "n6"):
        import anneal_refs as AR
        return AR.anneal_input(name)[1]
    if name == "bd12":
        import bd_refs as BD
        return BD.learner_input()[1]
    return LR.learning_input(name)[1]


def run_specs(name):
    """The commands of fixture `name`, as dicts: kind, criterion, seed, start (parent lists) and the kind's arguments."""
    import bd_refs as BD
    table = input_table(name)
    n = table.n
    empty = LR.empty_graph(n)

    def run(kind, criterion=None, seed=0, start=None, **args):
        return dict(kind=kind, criterion=criterion, seed=seed, start=[list(p) for p in (empty if start is None else start)], **args)
    if name == "n5":
        chain = [[], [0], [0, 1], [], [2, 3]]
        sparse = [[1, 2, 3, 4], [], [], [], []]   # the widest family of node 0: 48 parent configurations, all of them seen
        runs = [run("make_cpt", start=chain), run("make_cpt", start=sparse), run("make_cpt")]
        for c in ("aic", "mdl"):
            runs += [run("score", c, start=chain), run("score", c, start=chain, vertexes=[4, 0, 2]), run("score", c, start=sparse, vertexes=[0]),
                     run("greedy_all", c, seed=7), run("greedy_vertexes", c, seed=11, start=[[], [], [1], [], []], vertexes=[3, 4, 1, 0]),
                     run("greedy_hint", c, seed=5, hint=([0, 1], [2, 3, 4])),
                     run("k2", c, seed=5, precondition={3: [0, 1, 2], 1: [4]}), run("k2", c, seed=9, precondition={}),
                     run("brute_vertexes", c, vertexes=BD.BRUTE_VERTEXES), run("brute_vertexes", c, start=[[], [], [], [2], []], vertexes=[3, 0, 4]),
                     run("brute_hint", c, start=BD.BRUTE_HINT_START, hint=BD.BRUTE_HINT), run("brute_hint", c, hint=([0, 2], [1, 3, 4])),
                     run("stepwise", c, seed=3, between_seed=4, size=2), run("stepwise", c, seed=8, between_seed=1, size=3)]
        runs.append(run("brute_all", "aic"))   # operator()(graph): the five vertexes in node order
        return table, runs
    if name == "n6":
        dense = [[], [0], [0, 1], [1, 2], [3], [0, 2, 3, 4]]   # node 1 has arity 1
        unseen = [[2, 3, 4, 5], [0, 2, 3, 4, 5], [], [], [], []]   # 1 of node 0's 120 and 11 of node 1's 240 configurations are never seen
        runs = [run("make_cpt", start=dense), run("make_cpt", start=unseen)]
        for c in ("aic", "mdl"):
            runs += [run("score", c, start=dense), run("score", c, start=dense, vertexes=[5, 1]),
                     run("greedy_all", c, seed=2), run("greedy_hint", c, seed=6, hint=([1, 3, 5], [0, 2, 4])),
                     run("k2", c, seed=4, precondition={5: [1], 0: [2, 3]}),
                     run("brute_vertexes", c, vertexes=[5, 1, 3, 0]), run("brute_hint", c, hint=([1, 4], [0, 5])),
                     run("stepwise", c, seed=12, between_seed=13, size=2), run("stepwise", c, seed=1, between_seed=2, size=4)]
        return table, runs
    if name == "bd12":
        fitted = [[], [0], [], [1, 2], [3], [0, 4], [], [5, 6], [3, 7], [8], [2, 9], [4, 6, 10]]
        wide = [[], [0, 2, 3, 4, 5, 6]] + LR.empty_graph(9) + [[0, 1, 2, 3, 4, 5, 6]]   # rows of 1/3 and of 1/2 that no sample shows
        runs = [run("make_cpt", start=fitted), run("make_cpt", start=wide)]
        for c in ("aic", "mdl"):
            runs += [run("score", c, start=fitted), run("score", c, start=fitted, vertexes=[11, 3, 7]),
                     run("greedy_all", c, seed=BD.GREEDY_SEED), run("greedy_hint", c, seed=BD.HINT_SEED, hint=(BD.HINT_PARENTS, BD.HINT_CHILDREN)),
                     run("k2", c, seed=BD.K2_SEED, precondition=BD.K2_PRECONDITION),
                     run("stepwise", c, seed=17, between_seed=18, size=3)]
        return table, runs
    if name == "alarm2k_mdl":
        # greedy only: the reference's K2 on this input evaluates 1 287 graphs and takes ten minutes (EXPERIMENTS R15.3)
        return table, [run("greedy_all", "mdl", seed=21)]
    raise KeyError(name)


def command_of(spec):
    """The driver's command tokens for a run spec."""
    kind, c = spec["kind"], spec["criterion"]

    def nodes(vs):
        return [len(vs)] + [int(v) for v in vs]
    if kind == "make_cpt":
        return ["make_cpt"]
    if kind == "score":
        return ["score", c] + ([-1] if spec.get("vertexes") is None else nodes(spec["vertexes"]))
    if kind == "greedy_all":
        return ["greedy", c, spec["seed"], "all"]
    if kind == "greedy_vertexes":
        return ["greedy", c, spec["seed"], "vertexes"] + nodes(spec["vertexes"])
    if kind == "greedy_hint":
        return ["greedy", c, spec["seed"], "hint"] + nodes(spec["hint"][0]) + nodes(spec["hint"][1])
    if kind == "k2":
        pre = spec["precondition"]
        return ["k2", c, spec["seed"], len(pre)] + [x for t in pre for x in [int(t)] + nodes(pre[t])]
    if kind == "brute_all":
        return ["brute", c, "all"]
    if kind == "brute_vertexes":
        return ["brute", c, "vertexes"] + nodes(spec["vertexes"])
    if kind == "brute_hint":
        return ["brute", c, "hint"] + nodes(spec["hint"][0]) + nodes(spec["hint"][1])
    if kind == "stepwise":
        return ["stepwise", c, spec["seed"], spec["between_seed"], spec["size"]]
    raise KeyError(kind)


# ---- packing: a fixture is arrays only --------------------------------------------------------------------------

def _ragged(lists, dtype=np.int16):
    ptr = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.asarray([int(v) for x in lists for v in x], dtype=dtype)
    return ptr, flat


def _unragged(ptr, flat):
    return [[int(x) for x in flat[ptr[i]:ptr[i + 1]]] for i in range(len(ptr) - 1)]


def pack_run(spec, out):
    """Arrays of one run: its spec and the driver's JSON `out`."""
    d = {"kind": np.str_(spec["kind"]), "criterion": np.str_(spec["criterion"] or ""), "seed": np.int64(spec["seed"]),
         "between_seed": np.int64(spec.get("between_seed", 0)), "size": np.int64(spec.get("size", 0))}
    d["start_ptr"], d["start_idx"] = _ragged(spec["start"])
    args, has_vertexes = [], spec.get("vertexes") is not None
    if has_vertexes:
        args = [spec["vertexes"]]
    elif "hint" in spec:
        args = [spec["hint"][0], spec["hint"][1]]
    elif "precondition" in spec:
        args = [list(spec["precondition"].keys())] + [list(v) for v in spec["precondition"].values()]
    d["has_vertexes"] = np.bool_(has_vertexes)
    d["arg_ptr"], d["arg_idx"] = _ragged(args)
    if spec["kind"] == "make_cpt":
        d["cpt"] = np.asarray(out["cpt"], np.float64)
        return d
    d["value"] = np.float64(out["value"])
    d["final_edges"] = np.asarray(out["final_edges"], np.uint8).reshape(-1, 2)
    evals = out["evals"]
    d["eval_ptr"], flat = _ragged([e["edges"] for e in evals], np.uint8)
    d["eval_edges"] = flat.reshape(-1, 2)
    d["eval_ptr"] = d["eval_ptr"] // 2
    d["eval_value"] = np.asarray([e["value"] for e in evals], np.float64)
    d["eval_has_vertexes"] = np.asarray(["vertexes" in e for e in evals], np.bool_)
    d["eval_vptr"], d["eval_vtx"] = _ragged([e.get("vertexes", []) for e in evals], np.uint8)
    d["inner_ptr"], d["inner_idx"] = _ragged([c["first"] for c in out["inner_calls"]])
    d["inner_begin"] = np.asarray([c["eval_begin"] for c in out["inner_calls"]], np.int32)
    d["between_pptr"], d["between_pidx"] = _ragged([c["first"] for c in out["between_calls"]])
    d["between_cptr"], d["between_cidx"] = _ragged([c["second"] for c in out["between_calls"]])
    d["between_begin"] = np.asarray([c["eval_begin"] for c in out["between_calls"]], np.int32)
    return d


def parents_of(n, edges):
    """Parent lists (increasing) from [(parent, child), ...]."""
    out = [[] for _ in range(n)]
    for p, c in edges:
        out[int(c)].append(int(p))
    return [sorted(x) for x in out]


class Run:
    """One command of a fixture.  `evals`: [(edge set, vertexes or None, value)] in the order the reference evaluated."""

    def __init__(self, n, d):
        self.n = n
        self.kind, self.criterion, self.seed = str(d["kind"]), str(d["criterion"]), int(d["seed"])
        self.between_seed, self.size = int(d["between_seed"]), int(d["size"])
        self.start = _unragged(d["start_ptr"], d["start_idx"])
        args = _unragged(d["arg_ptr"], d["arg_idx"])
        self.vertexes = args[0] if bool(d["has_vertexes"]) else None
        self.hint = (args[0], args[1]) if self.kind.endswith("_hint") else None
        self.precondition = {t: args[1 + i] for i, t in enumerate(args[0])} if self.kind == "k2" and args else {}
        if self.kind == "make_cpt":
            self.cpt = np.asarray(d["cpt"])
            return
        self.value = float(d["value"])
        self.final = parents_of(n, d["final_edges"])
        ptr, edges, vptr, vtx = d["eval_ptr"], d["eval_edges"], d["eval_vptr"], d["eval_vtx"]
        self.evals = []
        for j in range(len(ptr) - 1):
            es = frozenset((int(p), int(c)) for p, c in edges[ptr[j]:ptr[j + 1]])
            vs = [int(v) for v in vtx[vptr[j]:vptr[j + 1]]] if bool(d["eval_has_vertexes"][j]) else None
            self.evals.append((es, vs, float(d["eval_value"][j])))
        self.inner_calls = list(zip(_unragged(d["inner_ptr"], d["inner_idx"]), [int(b) for b in d["inner_begin"]]))
        self.between_calls = list(zip(_unragged(d["between_pptr"], d["between_pidx"]), _unragged(d["between_cptr"], d["between_cidx"]),
                                      [int(b) for b in d["between_begin"]]))

    def __repr__(self):
        return f"{self.kind}/{self.criterion or '-'}/seed{self.seed}"


_LOADED = {}


def load(name):
    """(learning_refs.Table, [Run]) of tests/golden/learn_<name>.npz; cached per process, never modified."""
    if name not in _LOADED:
        z = np.load(os.path.join(GOLDEN, f"learn_{name}.npz"))
        table = LR.Table(z["patterns"], z["counts"], z["k"])
        runs = []
        for i in range(int(z["n_runs"])):
            prefix = f"run{i}_"
            runs.append(Run(table.n, {key[len(prefix):]: z[key] for key in z.files if key.startswith(prefix)}))
        _LOADED[name] = (table, runs)
    return _LOADED[name]


def all_runs(kinds=None):
    """[(fixture name, run index)] of every run of every fixture (of the given kinds): the parameter lists of the tests."""
    out = []
    for name in fixture_names():
        for i, r in enumerate(load(name)[1]):
            if kinds is None or r.kind in kinds:
                out.append((name, i))
    return out


# ---- reading a log -----------------------------------------------------------------------------------------------

def edge_set(parents):
    return frozenset((int(p), c) for c, ps in enumerate(parents) for p in ps)


def try_segment(n, evals, begin, end, end_graph):
    """A stretch of the log written by greedy's / k2_algorithm's loop: evals[begin] is the graph the loop starts from (eval_now /
    eval_best), every later entry the current graph plus ONE edge.  Whether the reference kept that edge is read off the NEXT
    logged graph (the graph after the loop, `end_graph`, for the last one), not off the values.  Returns [(child, candidate,
    value of the candidate graph, value it was compared with, kept, parent lists before)]."""
    cur, now = evals[begin][0], evals[begin][2]
    out = []
    for j in range(begin + 1, end):
        es, _, value = evals[j]
        extra = es - cur
        assert cur <= es and len(extra) == 1, f"log entry {j} is not the current graph plus one edge"
        (p, c), = extra
        nxt = evals[j + 1][0] if j + 1 < end else end_graph
        kept = (p, c) in nxt
        out.append((c, p, value, now, kept, parents_of(n, cur)))
        if kept:
            cur, now = es, value
    assert cur == end_graph, "the log does not end in the final graph"
    return out


def orders_of(decisions):
    """(children, candidates per child) in the order of the log: consecutive entries with the same child are one visit."""
    children, tails = [], []
    for c, p, *_ in decisions:
        if not children or children[-1] != c:
            children.append(c)
            tails.append([])
        tails[-1].append(p)
    return children, tails


def stepwise_segments(run):
    """The stretches of a stepwise log: [("inner", cluster, begin, end)], [("between", parents, children, begin, end)]."""
    marks = [("inner", c, None, b) for c, b in run.inner_calls] + [("between", p, c, b) for p, c, b in run.between_calls]
    ends = [m[3] for m in marks[1:]] + [len(run.evals)]
    return [m + (e,) for m, e in zip(marks, ends)]


def plan_of(run):
    """stepwise_structure's (clusters, [(parent index, child index)]) from the lists its learners were called with: the merge rule
    (stepwise_structure.hpp:95-103: both clusters leave, parent + child joins at the end) turns the logged node lists into indexes."""
    clusters = [list(c) for c, _ in run.inner_calls]
    cl, pairs = [list(c) for c in clusters], []
    for ps, cs, _ in run.between_calls:
        pi, ci = cl.index(ps), cl.index(cs)
        pairs.append((pi, ci))
        cl = [x for i, x in enumerate(cl) if i not in (pi, ci)] + [ps + cs]
    assert len(cl) == 1
    return clusters, pairs


def exact_terms(table, parents, vertexes=None):
    """The log-likelihood of G with fitted CPTs in EXACT arithmetic, as integers: it is sum over the cells of N log N minus sum
    over the parent configurations of R log R (R the row total), so {m: how often m log m enters, signed} determines it.  Equal
    dicts mean equal likelihoods with no rounding involved (the converse is not claimed)."""
    out = {}
    for v in (range(table.n) if vertexes is None else vertexes):
        N = LR.family_counts(table.pats, table.counts, table.k, int(v), parents[int(v)]).reshape(-1, int(table.k[int(v)]))
        for m in N[N > 1].tolist():
            out[m] = out.get(m, 0) + 1
        for m in N.sum(axis=1, dtype=np.uint64).tolist():
            if m > 1:
                out[m] = out.get(m, 0) - 1
    return {m: c for m, c in out.items() if c}


def exact_tie(table, a, b, vertexes=None) -> bool:
    """Two graphs whose AIC and MDL are EQUAL in exact arithmetic: the same parameter count and the same exact likelihood (over
    `vertexes`).  Markov-equivalent graphs (a -> b against b -> a) and graphs that differ by an edge at a node of arity 1 are
    such pairs.  Which of the two a `<` prefers is decided by the rounding of whoever computes it, on any input and any seed."""
    pa = sum(LR.family_params(table.k, v, ps) for v, ps in enumerate(a))
    pb = sum(LR.family_params(table.k, v, ps) for v, ps in enumerate(b))
    return pa == pb and exact_terms(table, a, vertexes) == exact_terms(table, b, vertexes)


def restated_value(table, parents, criterion, vertexes=None):
    """The project's restatement of eval_(graph[, vertexes]) with fitted CPTs: score_arith over Table.libm_ll."""
    vs = range(table.n) if vertexes is None else vertexes
    params = sum(LR.family_params(table.k, v, ps) for v, ps in enumerate(parents))
    return LR.score_arith([table.libm_ll(int(v), parents[int(v)]) for v in vs], params, criterion, table.total)
