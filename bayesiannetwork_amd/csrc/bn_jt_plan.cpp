// bn_jt_plan.cpp -- the junction-tree planner (bn_jt_plan.hpp).  Host arithmetic only.
#include "bn_jt_plan.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <set>
#include <tuple>

namespace bnmi {
namespace {

using Adj = std::vector<std::vector<int32_t>>;

bool adjacent(const Adj& adj, int32_t a, int32_t b) { return std::binary_search(adj[a].begin(), adj[a].end(), b); }
void link(Adj& adj, int32_t a, int32_t b) {
    adj[a].insert(std::lower_bound(adj[a].begin(), adj[a].end(), b), b);
    adj[b].insert(std::lower_bound(adj[b].begin(), adj[b].end(), a), a);
}
void unlink_from(Adj& adj, int32_t a, int32_t gone) {
    auto it = std::lower_bound(adj[a].begin(), adj[a].end(), gone);
    if (it != adj[a].end() && *it == gone) adj[a].erase(it);
}
int64_t fill_of(const Adj& adj, int32_t v) {
    int64_t f = 0;
    const std::vector<int32_t>& nb = adj[v];
    for (size_t i = 0; i < nb.size(); ++i)
        for (size_t j = i + 1; j < nb.size(); ++j) f += adjacent(adj, nb[i], nb[j]) ? 0 : 1;
    return f;
}
double weight_of(const Adj& adj, const int32_t* k, int32_t v) {
    double w = double(k[v]);
    for (int32_t u : adj[v]) w *= double(k[u]);
    return w;
}

// entry e of a table over `vars` (ascending, first most significant) -> sum over the variables of digit x weight, for every e
void project(const std::vector<int32_t>& vars, const int32_t* k, const std::vector<int32_t>& weight, int32_t* out, int64_t size) {
    const size_t m = vars.size();
    std::vector<int32_t> digit(m, 0);
    int32_t cur = 0;
    for (int64_t e = 0; e < size; ++e) {
        out[e] = cur;
        for (size_t i = m; i-- > 0;) {
            cur += weight[i];
            if (++digit[i] < k[vars[i]]) break;
            cur -= weight[i] * k[vars[i]];
            digit[i] = 0;
        }
    }
}

// strides of `vars` inside a table over them
std::vector<int32_t> strides_of(const std::vector<int32_t>& vars, const int32_t* k) {
    std::vector<int32_t> s(vars.size(), 1);
    for (size_t i = vars.size(); i-- > 1;) s[i - 1] = s[i] * k[vars[i]];
    return s;
}

// the tables of a sum over clique `big` onto its subset `sub`: the first term's offset per entry of `sub`, the terms' offsets
void sum_tables(const std::vector<int32_t>& big, const std::vector<int32_t>& sub, const int32_t* k, int32_t* base, std::vector<int32_t>& res) {
    const std::vector<int32_t> bs = strides_of(big, k);
    std::vector<int32_t> sub_w, rest, rest_w;
    int64_t sub_size = 1, rest_size = 1;
    for (size_t i = 0; i < big.size(); ++i) {
        if (std::binary_search(sub.begin(), sub.end(), big[i])) { sub_w.push_back(bs[i]); sub_size *= k[big[i]]; }
        else { rest.push_back(big[i]); rest_w.push_back(bs[i]); rest_size *= k[big[i]]; }
    }
    project(sub, k, sub_w, base, sub_size);
    const size_t at = res.size();
    res.resize(at + size_t(rest_size));
    project(rest, k, rest_w, res.data() + at, rest_size);
}

}  // namespace

void jt_apply_budget(JtPlan& p, int64_t scratch_cells) {
    if (!p.built) return;
    p.ok = p.state_cells <= scratch_cells;
    p.why = p.ok ? std::string()
                 : "the state of one evidence set, " + std::to_string(p.state_cells) + " doubles (" + std::to_string(p.nc) + " cliques, " +
                       std::to_string(p.pot_cells) + " potential and " + std::to_string(p.sep_cells) + " separator entries), is above the scratch budget of " +
                       std::to_string(scratch_cells) + " (option jt_scratch_cells)";
}

int jt_form(const JtPlan& p, int option) {
    if (!p.ok) return 0;
    const bool lds = p.state_cells <= kJtLdsCells;
    if (option == 1) return lds ? 1 : 0;
    if (option == 2) return 2;
    return lds ? 1 : 2;
}

void build_jt_plan(int32_t n, const int32_t* k, const int32_t* in_ptr, const int32_t* in_idx, const int64_t* cpt_off, int64_t scratch_cells,
                   JtPlan& out) {
    out = JtPlan();
    JtPlan& P = out;
    P.n = n;
    if (n < 1) { P.why = "the network has no node"; return; }
    // ---- the moral graph
    Adj adj(static_cast<size_t>(n));
    for (int32_t v = 0; v < n; ++v)
        for (int32_t a = in_ptr[v]; a < in_ptr[v + 1]; ++a) {
            adj[v].push_back(in_idx[a]);
            adj[in_idx[a]].push_back(v);
            for (int32_t b = a + 1; b < in_ptr[v + 1]; ++b) {
                adj[in_idx[a]].push_back(in_idx[b]);
                adj[in_idx[b]].push_back(in_idx[a]);
            }
        }
    for (auto& a : adj) {
        std::sort(a.begin(), a.end());
        a.erase(std::unique(a.begin(), a.end()), a.end());
    }
    // ---- elimination: min-fill, then the smaller table, then the lower id
    using Key = std::tuple<int64_t, double, int32_t>;
    std::vector<Key> key(size_t(n), Key(0, 0.0, 0));
    std::set<Key> queue;
    for (int32_t v = 0; v < n; ++v) queue.insert(key[v] = Key(fill_of(adj, v), weight_of(adj, k, v), v));
    std::vector<std::vector<int32_t>> elim(static_cast<size_t>(n));   // elimination clique i: its variables, ascending
    std::vector<int32_t> pos(size_t(n), -1);
    std::vector<uint8_t> mark(size_t(n), 0);
    std::vector<int32_t> touched;
    P.order.reserve(static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) {
        const int32_t v = std::get<2>(*queue.begin());
        queue.erase(queue.begin());
        pos[v] = i;
        P.order.push_back(v);
        const std::vector<int32_t> nb = adj[v];
        std::vector<int32_t>& c = elim[i];
        c = nb;
        c.insert(std::lower_bound(c.begin(), c.end(), v), v);
        double size = 1.0;
        for (int32_t u : c) size *= double(k[u]);
        if (size > double(kJtMaxClique)) {
            char buf[64];
            std::snprintf(buf, sizeof buf, "%.0f", size);
            P.why = "the elimination clique of node " + std::to_string(v) + " has " + std::to_string(c.size()) + " variables and " + buf +
                    " entries: above the limit of " + std::to_string(kJtMaxClique) + " entries per clique table";
            return;
        }
        bool added = false;
        for (size_t a = 0; a < nb.size(); ++a)
            for (size_t b = a + 1; b < nb.size(); ++b)
                if (!adjacent(adj, nb[a], nb[b])) { link(adj, nb[a], nb[b]); added = true; }
        touched.clear();
        for (int32_t u : nb) {
            unlink_from(adj, u, v);
            if (!mark[u]) { mark[u] = 1; touched.push_back(u); }
        }
        if (added)
            for (int32_t u : nb)
                for (int32_t w : adj[u])
                    if (!mark[w]) { mark[w] = 1; touched.push_back(w); }
        for (int32_t u : touched) {
            mark[u] = 0;
            queue.erase(key[u]);
            queue.insert(key[u] = Key(fill_of(adj, u), weight_of(adj, k, u), u));
        }
        adj[v].clear();
    }
    // ---- the maximal cliques and their forest.  up[i]: the elimination clique that holds clique i without its own node -- that of
    // the earliest-eliminated other member.  Clique j is not maximal iff a clique i below it (up[i] == j) has one variable more; it
    // is then absorbed by the first such i.
    std::vector<int32_t> up(size_t(n), -1), into(size_t(n), -1);
    for (int32_t i = 0; i < n; ++i) {
        int32_t best = n;
        for (int32_t u : elim[i])
            if (pos[u] > i) best = std::min(best, pos[u]);
        up[i] = best == n ? -1 : best;
    }
    for (int32_t i = 0; i < n; ++i)
        if (up[i] >= 0 && into[up[i]] < 0 && elim[i].size() == elim[up[i]].size() + 1) into[up[i]] = i;
    auto rep = [&](int32_t i) {
        while (into[i] >= 0) i = into[i];
        return i;
    };
    std::vector<int32_t> kept;
    for (int32_t i = 0; i < n; ++i)
        if (into[i] < 0) kept.push_back(i);
    const int32_t nc = int32_t(kept.size());
    std::vector<int32_t> kid(size_t(n), -1);   // elimination index -> position in `kept`
    for (int32_t c = 0; c < nc; ++c) kid[kept[c]] = c;
    std::vector<std::vector<int32_t>> tree(static_cast<size_t>(nc));
    for (int32_t c = 0; c < nc; ++c) {
        int32_t p = up[kept[c]];
        while (p >= 0 && rep(p) == kept[c]) p = up[p];
        if (p < 0) continue;
        const int32_t q = kid[rep(p)];
        tree[c].push_back(q);
        tree[q].push_back(c);
    }
    for (auto& t : tree) std::sort(t.begin(), t.end());
    // ---- every tree rooted at its centre (the middle of a longest path), levels, the final numbering
    std::vector<int32_t> dist(size_t(nc), -1), from(size_t(nc), -1), bfs;
    auto sweep = [&](int32_t s) {   // breadth-first from s: the farthest clique (the first one reached at that distance)
        bfs.assign(1, s);
        dist[s] = 0;
        from[s] = -1;
        int32_t far = s;
        for (size_t h = 0; h < bfs.size(); ++h) {
            const int32_t x = bfs[h];
            if (dist[x] > dist[far]) far = x;
            for (int32_t y : tree[x])
                if (y != from[x]) { dist[y] = dist[x] + 1; from[y] = x; bfs.push_back(y); }
        }
        return far;
    };
    std::vector<int32_t> roots;
    std::vector<uint8_t> seen(size_t(nc), 0);
    for (int32_t s = 0; s < nc; ++s) {
        if (seen[s]) continue;
        const int32_t a = sweep(s);
        for (int32_t x : bfs) seen[x] = 1;
        int32_t b = sweep(a);
        for (int32_t steps = dist[b] / 2; steps > 0; --steps) b = from[b];
        roots.push_back(b);
    }
    std::vector<int32_t> new_of(size_t(nc), -1), old_of, par_old(size_t(nc), -1);
    old_of.reserve(static_cast<size_t>(nc));
    std::vector<int32_t> lvl_ptr(1, 0);
    for (int32_t r : roots) { new_of[r] = int32_t(old_of.size()); old_of.push_back(r); }
    P.parent.assign(size_t(nc), -1);
    P.level.assign(size_t(nc), 0);
    std::vector<int32_t> child_lo(size_t(nc), 0), child_hi(size_t(nc), 0);
    for (size_t lo = 0; lo < old_of.size();) {
        const size_t hi = old_of.size();
        lvl_ptr.push_back(int32_t(hi));
        for (size_t c = lo; c < hi; ++c) {
            child_lo[c] = int32_t(old_of.size());
            for (int32_t y : tree[old_of[c]])
                if (y != par_old[old_of[c]]) {
                    par_old[y] = old_of[c];
                    new_of[y] = int32_t(old_of.size());
                    P.parent[old_of.size()] = int32_t(c);
                    P.level[old_of.size()] = int32_t(lvl_ptr.size()) - 1;
                    old_of.push_back(y);
                }
            child_hi[c] = int32_t(old_of.size());
        }
        lo = hi;
    }
    P.nc = nc;
    P.nlev = int32_t(lvl_ptr.size()) - 1;
    // ---- variables, separators, sizes
    P.var_ptr.assign(1, 0);
    P.sep_ptr.assign(1, 0);
    std::vector<int64_t> size(size_t(nc), 1), sep_size(size_t(nc), 1);
    for (int32_t c = 0; c < nc; ++c) {
        const std::vector<int32_t>& vs = elim[kept[old_of[c]]];
        P.vars.insert(P.vars.end(), vs.begin(), vs.end());
        P.var_ptr.push_back(int32_t(P.vars.size()));
        for (int32_t u : vs) size[c] *= k[u];
        if (P.parent[c] >= 0) {
            const std::vector<int32_t>& ps = elim[kept[old_of[P.parent[c]]]];
            for (int32_t u : vs)
                if (std::binary_search(ps.begin(), ps.end(), u)) { P.sep_vars.push_back(u); sep_size[c] *= k[u]; }
        }
        P.sep_ptr.push_back(int32_t(P.sep_vars.size()));
        P.pot_cells += size[c];
        P.sep_cells += sep_size[c];
        if (size[c] > P.max_clique) { P.max_clique = size[c]; P.max_clique_vars = int32_t(vs.size()); }
    }
    int64_t N = 0;
    for (int32_t v = 0; v < n; ++v) N += k[v];
    P.N = int32_t(N);
    P.state_cells = P.pot_cells + P.sep_cells + N + nc;
    // ---- CPTs and homes
    P.cpt_clique.assign(size_t(n), -1);
    P.home.assign(size_t(n), -1);
    for (int32_t v = 0; v < n; ++v) {
        int32_t first = pos[v];
        for (int32_t a = in_ptr[v]; a < in_ptr[v + 1]; ++a) first = std::min(first, pos[in_idx[a]]);
        P.cpt_clique[v] = new_of[kid[rep(first)]];
    }
    for (int32_t c = 0; c < nc; ++c)
        for (int32_t a = P.var_ptr[c]; a < P.var_ptr[c + 1]; ++a) {
            int32_t& h = P.home[P.vars[a]];
            if (h < 0 || size[c] < size[h]) h = c;
        }
    P.built = true;
    jt_apply_budget(P, scratch_cells);
    if (!P.ok) return;
    // ---- item tables
    P.cliques.assign(size_t(nc), JtClique());
    P.ent_clique.resize(size_t(P.pot_cells));
    P.dn_map.resize(size_t(P.pot_cells));
    P.sep_clique.resize(size_t(P.sep_cells));
    P.c_base.resize(size_t(P.sep_cells));
    P.p_base.assign(size_t(P.sep_cells), 0);
    std::vector<std::vector<int32_t>> cv(static_cast<size_t>(nc)), sv(static_cast<size_t>(nc));
    int32_t pot_at = 0, sep_at = 0;
    for (int32_t c = 0; c < nc; ++c) {
        cv[c].assign(P.vars.begin() + P.var_ptr[c], P.vars.begin() + P.var_ptr[c + 1]);
        sv[c].assign(P.sep_vars.begin() + P.sep_ptr[c], P.sep_vars.begin() + P.sep_ptr[c + 1]);
        JtClique& q = P.cliques[c];
        q.pot_off = pot_at; q.size = int32_t(size[c]);
        q.sep_off = sep_at; q.sep_size = int32_t(sep_size[c]);
        q.parent = P.parent[c]; q.level = P.level[c];
        q.child_lo = child_lo[c]; q.child_hi = child_hi[c];
        pot_at += q.size; sep_at += q.sep_size;
    }
    for (int32_t c = 0; c < nc; ++c) {
        JtClique& q = P.cliques[c];
        std::fill(P.ent_clique.begin() + q.pot_off, P.ent_clique.begin() + q.pot_off + q.size, c);
        std::fill(P.sep_clique.begin() + q.sep_off, P.sep_clique.begin() + q.sep_off + q.sep_size, c);
        const std::vector<int32_t> ss = strides_of(sv[c], k);
        auto weights_in = [&](const std::vector<int32_t>& big) {   // a clique's variables weighted by their stride in this separator
            std::vector<int32_t> w(big.size(), 0);
            for (size_t i = 0; i < big.size(); ++i) {
                auto it = std::lower_bound(sv[c].begin(), sv[c].end(), big[i]);
                if (it != sv[c].end() && *it == big[i]) w[i] = ss[size_t(it - sv[c].begin())];
            }
            return w;
        };
        project(cv[c], k, weights_in(cv[c]), P.dn_map.data() + q.pot_off, q.size);
        q.cres_off = int32_t(P.c_res.size());
        sum_tables(cv[c], sv[c], k, P.c_base.data() + q.sep_off, P.c_res);
        q.cres_cnt = int32_t(P.c_res.size()) - q.cres_off;
        q.pres_off = int32_t(P.p_res.size());
        q.up_off = int32_t(P.up_map.size());
        if (q.parent >= 0) {
            const std::vector<int32_t>& pv = cv[q.parent];
            sum_tables(pv, sv[c], k, P.p_base.data() + q.sep_off, P.p_res);
            P.up_map.resize(size_t(q.up_off) + size_t(size[q.parent]));
            project(pv, k, weights_in(pv), P.up_map.data() + q.up_off, size[q.parent]);
        }
        q.pres_cnt = int32_t(P.p_res.size()) - q.pres_off;
    }
    P.levels.assign(size_t(P.nlev), JtLevel());
    for (int32_t l = 0; l < P.nlev; ++l) {
        JtLevel& L = P.levels[l];
        L.c_lo = lvl_ptr[l]; L.c_hi = lvl_ptr[l + 1];
        const JtClique &a = P.cliques[L.c_lo], &b = P.cliques[L.c_hi - 1];
        L.pot_lo = a.pot_off; L.pot_hi = b.pot_off + b.size;
        L.sep_lo = a.sep_off; L.sep_hi = b.sep_off + b.sep_size;
    }
    // nodes: home digit, belief offset; the cliques' home lists (ascending node id: nodes are visited in that order)
    P.nodes.assign(size_t(n), JtNode());
    P.elem_node.resize(size_t(N));
    std::vector<std::vector<int32_t>> homed(static_cast<size_t>(nc));
    int32_t bel = 0;
    for (int32_t v = 0; v < n; ++v) {
        const int32_t h = P.home[v];
        const std::vector<int32_t> hs = strides_of(cv[h], k);
        const size_t at = size_t(std::lower_bound(cv[h].begin(), cv[h].end(), v) - cv[h].begin());
        P.nodes[v] = JtNode{h, hs[at], k[v], bel};
        for (int32_t x = 0; x < k[v]; ++x) P.elem_node[size_t(bel + x)] = v;
        bel += k[v];
        homed[h].push_back(v);
    }
    for (int32_t c = 0; c < nc; ++c) {
        P.cliques[c].home_lo = int32_t(P.home_nodes.size());
        P.home_nodes.insert(P.home_nodes.end(), homed[c].begin(), homed[c].end());
        P.cliques[c].home_hi = int32_t(P.home_nodes.size());
    }
    // the CPTs of every clique, ascending node id, each with its family's digits
    std::vector<std::vector<int32_t>> tabs(static_cast<size_t>(nc));
    for (int32_t v = 0; v < n; ++v) tabs[P.cpt_clique[v]].push_back(v);
    P.asg_ptr.assign(1, 0);
    for (int32_t c = 0; c < nc; ++c) {
        const std::vector<int32_t> cs = strides_of(cv[c], k);
        for (int32_t v : tabs[c]) {
            JtAsg a{cpt_off[v], v, int32_t(P.fam.size()), 0, 0};
            int32_t cstride = 1;
            auto member = [&](int32_t u) {
                const size_t at = size_t(std::lower_bound(cv[c].begin(), cv[c].end(), u) - cv[c].begin());
                P.fam.push_back(JtFam{cs[at], k[u], cstride});
                cstride *= k[u];
            };
            member(v);   // own state fastest, then the parents from the last (first parent most significant)
            for (int32_t e = in_ptr[v + 1]; e-- > in_ptr[v];) member(in_idx[e]);
            a.fam_hi = int32_t(P.fam.size());
            P.asg.push_back(a);
        }
        P.asg_ptr.push_back(int32_t(P.asg.size()));
    }
    // the families: per flat CPT entry (first parent most significant, own state last) the first term of its sum over the rest of
    // the clique, per node the offsets of the other terms -- the clique's variables outside the family, so ascending entry index
    if (cpt_off[n] > int64_t(INT32_MAX)) return;
    P.families.assign(size_t(n), JtFamily());
    P.f_node.resize(size_t(cpt_off[n]));
    P.f_base.resize(size_t(cpt_off[n]));
    for (int32_t v = 0; v < n; ++v) {
        const int32_t c = P.cpt_clique[v];
        const std::vector<int32_t> cs = strides_of(cv[c], k);
        std::vector<int32_t> members(in_idx + in_ptr[v], in_idx + in_ptr[v + 1]), weight, rest, rest_w;
        members.push_back(v);
        for (int32_t u : members) weight.push_back(cs[size_t(std::lower_bound(cv[c].begin(), cv[c].end(), u) - cv[c].begin())]);
        int64_t rest_size = 1;
        for (size_t i = 0; i < cv[c].size(); ++i)
            if (std::find(members.begin(), members.end(), cv[c][i]) == members.end()) {
                rest.push_back(cv[c][i]);
                rest_w.push_back(cs[i]);
                rest_size *= k[cv[c][i]];
            }
        JtFamily& F = P.families[size_t(v)];
        F.pot_off = P.cliques[c].pot_off;
        F.cpt_lo = int32_t(cpt_off[v]);
        F.cpt_cnt = int32_t(cpt_off[v + 1] - cpt_off[v]);
        F.res_off = int32_t(P.f_res.size());
        F.res_cnt = int32_t(rest_size);
        std::fill(P.f_node.begin() + F.cpt_lo, P.f_node.begin() + F.cpt_lo + F.cpt_cnt, v);
        project(members, k, weight, P.f_base.data() + F.cpt_lo, F.cpt_cnt);
        P.f_res.resize(size_t(F.res_off) + size_t(rest_size));
        project(rest, k, rest_w, P.f_res.data() + F.res_off, rest_size);
    }
}

}  // namespace bnmi
