"""Host restatement of expectation-maximisation over belief propagation (bn_em_*, bayesiannetwork_amd/csrc/bn_em.hpp).  Plain numpy,
no GPU.  Everything is fp64 and every sum has a stated order, so the device results are compared bit for bit.

The table.   patterns [P][n] uint8, counts [P] uint64 (bn_fit_cpt's layout); a cell of MISSING (255) is not observed.
E-step, per pattern p, under the current tables theta:
  1. every observed node gets a one-hot evidence vector (1.0 at its state);
  2. ``bp_run``: the sum-product loop of belief_propagation.hpp:33-158 -- restated here once more because the family posteriors need
     the final pi(v) and lambda(v), which maxprod_refs.run does not return; tests/test_em_refs.py pins it bit for bit (beliefs,
     messages, sweeps) to maxprod_refs.run(mode="sum").  bp_max_sweeps == 0 is a cap of DEFAULT_CAP sweeps, not unbounded; a run cut by
     the cap is used as it stands and counted;
  3. from the state the run stopped in, for every node v with parents u_1 < ... < u_m, assignment a (first parent most significant)
     and own state i:   t'[a,i] = ((cpt[a,i] x pimsg(u_1->v)[a_1]) x ...) x pimsg(u_m->v)[a_m]
                        r[i]    = sum_a t'[a,i]            front to back in table order from +0.0
                        s       = sum_i r[i] x lambda(v)[i] left to right from +0.0
                        b[a,i]  = (t'[a,i] x lambda(v)[i]) / s
     (an evidence node's lambda(v) is its one-hot vector).  Where ``s > 0`` is false the family contributes nothing and is counted;
  4. E[q] = sum_p float(counts[p]) x b_p[q]: patterns in blocks of BLOCK = 256 consecutive indices, inside a block in increasing p from
     +0.0, the block sums in increasing block order from +0.0.  E depends on the ORDER of the rows.
M-step.  E' = E + prior; per CPT row tot = sum_i E'[a,i] left to right from +0.0; theta_new = E' / tot, or 1.0 / k[v] for the whole row
  where ``tot > 0`` is false.
Loop.    delta = max_q |theta_new[q] - theta[q]| (a NaN is dropped); stop after the iteration where delta < tol (strict) or after
  max_iters iterations.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxprod_refs  # noqa: E402
from maxprod_refs import _Net, _fold, _normalize  # noqa: E402
from bayesiannetwork_amd import Evidence, FlatModel  # noqa: E402

MISSING = 255
BLOCK = 256
DEFAULT_CAP = 10000
DBL_MIN = np.finfo(np.float64).tiny


def with_cpt(model, cpt):
    return FlatModel(model.k, model.in_ptr, model.in_idx, model.cpt_off, np.ascontiguousarray(cpt, dtype=np.float64).copy(), name=model.name)


def evidence_of(model, row):
    """The pattern row as hard evidence: observed nodes in increasing id, one-hot vectors."""
    d = {int(v): int(row[v]) for v in range(model.n) if int(row[v]) != MISSING}
    return Evidence.from_dict(model, d) if d else None


def bp_run(model, evidence=None, eps=1e-3, max_sweeps=0):
    """The sum-product loop with the state it stopped in: dict(sweeps, converged, residuals, pi [n] and lam [n] (the final pi(v),
    lambda(v)), pim [edges] and lkm [edges] (the final messages, CSR edge order), pi_msg / lambda_msg (the same, flat), beliefs)."""
    net = _Net(model)
    n, k = model.n, net.k
    cap = max_sweeps if max_sweeps > 0 else DEFAULT_CAP
    ev = evidence if evidence is not None else Evidence.none()
    pi = [np.ones(k[v]) for v in range(n)]
    lam = [np.ones(k[v]) for v in range(n)]
    for v in range(n):
        if not net.par[v]:
            pi[v] = net.cpt[v].reshape(-1).copy()
    frozen = [False] * n
    for j in range(ev.ne):
        v = int(ev.node[j])
        frozen[v] = True
        vec = np.asarray(ev.val[int(ev.off[j]):int(ev.off[j]) + k[v]], dtype=np.float64)
        pi[v], lam[v] = vec.copy(), vec.copy()
    n_edges = int(model.n_edges)
    pim = [np.ones(k[int(model.in_idx[e])]) for e in range(n_edges)]
    lkm = [np.ones(k[int(model.in_idx[e])]) for e in range(n_edges)]
    residuals = []
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        while True:
            npim, nlkm = [None] * n_edges, [None] * n_edges
            npi, nlam = [None] * n, [None] * n
            for v in range(n):
                m, e0 = len(net.par[v]), net.edge0[v]
                for j, p in enumerate(net.par[v]):              # pi-messages into v (:202-218)
                    out = pi[p].copy()
                    for (c, e) in net.children[p]:
                        if c != v:
                            out = out * lkm[e]
                    npim[e0 + j] = _normalize(out)
                base = net.cpt[v] * lam[v]                      # lambda-messages out of v (:240-266)
                for jt in range(m):
                    w = base
                    for j in range(m):
                        if j != jt:
                            shape = [1] * (m + 1)
                            shape[j] = -1
                            w = w * pim[e0 + j].reshape(shape)
                    w = np.moveaxis(np.moveaxis(w, jt, 0), -1, 1).reshape(k[net.par[v][jt]], -1)
                    nlkm[e0 + jt] = _normalize(_fold(w, "sum"))
                if frozen[v]:                                   # pi(v) (:174-200)
                    npi[v] = pi[v]
                else:
                    npi[v] = _normalize(_fold(_pi_terms(net, v, pim).reshape(-1, k[v]).T, "sum"))
                if frozen[v]:                                   # lambda(v) (:220-238)
                    nlam[v] = lam[v]
                else:
                    out = np.ones(k[v])
                    for (_, e) in net.children[v]:
                        out = out * lkm[e]
                    nlam[v] = _normalize(out)
            md = DBL_MIN                                        # :105-131, messages only; std::max drops a NaN
            for e in range(n_edges):
                for old, new in ((pim[e], npim[e]), (lkm[e], nlkm[e])):
                    d = np.abs(new - old)
                    d = d[~np.isnan(d)]
                    if d.size and d.max() > md:
                        md = float(d.max())
            pi, lam, pim, lkm = npi, nlam, npim, nlkm
            residuals.append(md)
            converged = md < eps                                # :147 strict <
            if converged or len(residuals) >= cap:
                break
        beliefs = [_normalize(pi[v] * lam[v]) for v in range(n)]
    flat = lambda vs: np.concatenate(vs) if vs else np.zeros(0)   # noqa: E731
    return {"net": net, "sweeps": len(residuals), "converged": converged, "residuals": np.asarray(residuals), "pi": pi, "lam": lam,
            "pim": pim, "lkm": lkm, "pi_msg": flat(pim), "lambda_msg": flat(lkm), "beliefs": flat(beliefs)}


def _pi_terms(net, v, pim):
    """t'[a..., i]: cpt x the parents' pi-messages, ascending -- the terms pi(v)[i]'s sum adds."""
    m, e0 = len(net.par[v]), net.edge0[v]
    val = net.cpt[v]
    for j in range(m):
        shape = [1] * (m + 1)
        shape[j] = -1
        val = val * pim[e0 + j].reshape(shape)
    return val


def family_posteriors(model, run):
    """(b [entries] in the flat CPT layout, number of families with ``s > 0`` false) from the state bp_run stopped in."""
    net = run["net"]
    out = np.zeros(int(model.cpt_off[-1]))
    skipped = 0
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for v in range(model.n):
            kv = net.k[v]
            t = _pi_terms(net, v, run["pim"]).reshape(-1, kv)
            r = _fold(t.T, "sum")
            lam = run["lam"][v]
            s = 0.0
            for i in range(kv):
                s = s + r[i] * lam[i]
            if s > 0:
                out[int(model.cpt_off[v]):int(model.cpt_off[v + 1])] = ((t * lam) / s).reshape(-1)
            else:
                skipped += 1
    return out, skipped


def expected_counts(model, patterns, counts, bp_eps=1e-3, bp_max_sweeps=0):
    """One E-step under model.cpt: dict(E [entries], sweeps int32 [P], capped, skipped)."""
    patterns = np.asarray(patterns, np.uint8).reshape(-1, model.n)
    counts = np.asarray(counts, np.uint64)
    P, S = len(counts), int(model.cpt_off[-1])
    E = np.zeros(S)
    sweeps = np.zeros(P, np.int32)
    capped = skipped = 0
    memo = {}                                                   # rows that repeat give the same run
    for b0 in range(0, P, BLOCK):
        part = np.zeros(S)
        for p in range(b0, min(b0 + BLOCK, P)):
            key = patterns[p].tobytes()
            if key not in memo:
                run = bp_run(model, evidence_of(model, patterns[p]), bp_eps, bp_max_sweeps)
                b, sk = family_posteriors(model, run)
                memo[key] = (b, sk, run["sweeps"], not run["converged"])
            b, sk, sw, cut = memo[key]
            sweeps[p] = sw
            capped += int(cut)
            skipped += sk
            part = part + np.float64(counts[p]) * b
        E = E + part
    return {"E": E, "sweeps": sweeps, "capped": capped, "skipped": skipped}


def m_step(model, E, prior=0.0):
    out = np.zeros_like(E)
    for v in range(model.n):
        kv = int(model.k[v])
        rows = (E[int(model.cpt_off[v]):int(model.cpt_off[v + 1])] + prior).reshape(-1, kv)
        tot = np.zeros(rows.shape[0])
        for i in range(kv):
            tot = tot + rows[:, i]
        new = np.full(rows.shape, 1.0 / float(kv))
        ok = tot > 0
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            new[ok] = rows[ok] / tot[ok][:, None]
        out[int(model.cpt_off[v]):int(model.cpt_off[v + 1])] = new.reshape(-1)
    return out


def em_loop(model, e_step, max_iters, tol, prior, cpt_init, listed, summed):
    """The loop of both EM restatements (this module's and jtem_refs'): e_step(model under theta) -> dict with "E" and more.
    listed: {key of the result: key of the E-step's dict} collected per iteration beside E; summed: keys added up over the
    iterations.  dict(cpt, iters, deltas [iters], thetas [iters] (the tables after every iteration), E, the listed, the summed)."""
    theta = np.asarray(model.cpt if cpt_init is None else cpt_init, dtype=np.float64).copy()
    out = {"deltas": [], "thetas": [], "E": [], **{name: [] for name in listed}, **{name: 0 for name in summed}}
    for it in range(max_iters):
        e = e_step(with_cpt(model, theta))
        new = m_step(model, e["E"], prior)
        d = np.abs(new - theta)
        d = d[~np.isnan(d)]
        delta = float(d.max()) if d.size else 0.0
        theta = new
        out["deltas"].append(delta)
        out["thetas"].append(theta.copy())
        out["E"].append(e["E"])
        for name, key in listed.items():
            out[name].append(e[key])
        for name in summed:
            out[name] += e[name]
        if delta < tol:
            break
    out["cpt"], out["iters"], out["deltas"] = theta, len(out["deltas"]), np.asarray(out["deltas"])
    return out


def em_fit(model, patterns, counts, max_iters=100, tol=1e-6, bp_eps=1e-3, bp_max_sweeps=0, prior=0.0, cpt_init=None):
    """dict(cpt, iters, deltas [iters], thetas [iters] (the tables after every iteration), E and sweeps of every iteration, capped and
    skipped summed over the iterations)."""
    return em_loop(model, lambda m: expected_counts(m, patterns, counts, bp_eps, bp_max_sweeps), max_iters, tol, prior, cpt_init,
                   listed={"sweeps": "sweeps"}, summed=("capped", "skipped"))


def log_likelihood(model, patterns, counts):
    """Observed-data log-likelihood sum_p count_p x log P(e_p) on a polytree: exact two-pass sum-product in long double."""
    import exact_refs
    patterns = np.asarray(patterns, np.uint8).reshape(-1, model.n)
    total = np.longdouble(0)
    for row, c in zip(patterns, np.asarray(counts, np.uint64)):
        ev = evidence_of(model, row)
        if ev is None or int(c) == 0:
            continue                                            # log P(nothing observed) = 0
        total += np.longdouble(int(c)) * np.longdouble(exact_refs.exact_marginals(model, ev, bp_clamp=False)[1])
    return total


def random_positive_cpt(model, seed):
    """Strictly positive tables of the model's structure from another seed."""
    rng = np.random.default_rng(seed)
    cpt = np.zeros(int(model.cpt_off[-1]))
    for v in range(model.n):
        t = 0.1 + rng.random((int(model.cpt_off[v + 1] - model.cpt_off[v]) // int(model.k[v]), int(model.k[v])))
        cpt[int(model.cpt_off[v]):int(model.cpt_off[v + 1])] = (t / t.sum(axis=1, keepdims=True)).reshape(-1)
    return cpt


def sampled_table(model, n_samples, blank, seed):
    """n_samples forward samples with a fraction `blank` of the cells blanked, as distinct rows with counts (sorted: a fixed order)."""
    import exact_refs
    rng = np.random.default_rng(seed)
    rows = np.stack([exact_refs.forward_sample(model, rng) for _ in range(n_samples)]).astype(np.uint8)
    rows[rng.random(rows.shape) < blank] = MISSING
    pats, cnt = np.unique(rows, axis=0, return_counts=True)
    return np.ascontiguousarray(pats, dtype=np.uint8), cnt.astype(np.uint64)


# ---- the cases of "EM improves the likelihood" (tests/test_em_refs.py): (nodes, polytree seed, samples, blanked fraction, seed of the
# starting tables).  Chosen on the CPU: the restatement alone raises the observed-data log-likelihood at every one of 8 iterations.
# A case that fails is a test FAILURE, never a skip.
LIKELIHOOD_CASES = [(6, 1, 200, 0.25, 11), (8, 2, 200, 0.3, 12), (10, 3, 200, 0.4, 13)]


def likelihood_case(n, seed, n_samples, blank, init_seed):
    import exact_refs
    model = exact_refs.polytree(n, arities=(2, 3, 4), max_parents=3, seed=seed, name=f"em_polytree{n}_s{seed}")
    pats, cnt = sampled_table(model, n_samples, blank, seed=200 + seed)
    return model, pats, cnt, random_positive_cpt(model, init_seed)
