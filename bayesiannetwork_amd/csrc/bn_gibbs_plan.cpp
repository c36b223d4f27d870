// bn_gibbs_plan.cpp -- the planner of bn_gibbs_plan.hpp: moral graph, greedy colouring, slots, launch shape.  No HIP.
#include "bn_gibbs_plan.hpp"

#include <algorithm>

namespace bnmi {

void build_gibbs_plan(int32_t n, const int32_t* k, const int32_t* in_ptr, const int32_t* in_idx, const int64_t* cpt_off, GibbsPlan& out) {
    out = GibbsPlan();
    out.n = n;
    if (n > kGibbsMaxNodes) {
        out.why = "the network has " + std::to_string(n) + " nodes; this form of Gibbs sampling keeps a chain's states in LDS and takes at most " +
                  std::to_string(kGibbsMaxNodes);
        return;
    }
    int64_t cells = 0;
    for (int32_t v = 0; v < n; ++v) cells += k[v];
    if (cells > kGibbsMaxCells) {
        out.why = "the arities sum to " + std::to_string(cells) + "; this form of Gibbs sampling keeps a workgroup's histogram in LDS and takes at most " +
                  std::to_string(kGibbsMaxCells);
        return;
    }
    out.cells = int32_t(cells);

    // children of every node, ascending (nodes are visited in ascending index)
    std::vector<std::vector<int32_t>> kids(size_t(std::max(n, 0)));
    for (int32_t v = 0; v < n; ++v)
        for (int32_t e = in_ptr[v]; e < in_ptr[v + 1]; ++e) kids[size_t(in_idx[e])].push_back(v);

    // the moral graph: the members of every family are neighbours of each other
    std::vector<std::vector<int32_t>> adj(static_cast<size_t>(n));
    for (int32_t v = 0; v < n; ++v) {
        for (int32_t a = in_ptr[v]; a < in_ptr[v + 1]; ++a) {
            const int32_t p = in_idx[a];
            adj[size_t(v)].push_back(p);
            adj[size_t(p)].push_back(v);
            for (int32_t b = in_ptr[v]; b < in_ptr[v + 1]; ++b)
                if (b != a) adj[size_t(p)].push_back(in_idx[b]);
        }
    }
    // greedy colouring, ascending node index
    out.colour.assign(size_t(n), -1);
    std::vector<int32_t> seen;      // seen[c] == v + 1: a neighbour of v holds colour c
    for (int32_t v = 0; v < n; ++v) {
        for (int32_t u : adj[size_t(v)]) {
            const int32_t c = out.colour[size_t(u)];
            if (c < 0) continue;
            if (size_t(c) >= seen.size()) seen.resize(size_t(c) + 1, 0);
            seen[size_t(c)] = v + 1;
        }
        int32_t c = 0;
        while (size_t(c) < seen.size() && seen[size_t(c)] == v + 1) ++c;
        out.colour[size_t(v)] = c;
        out.n_colours = std::max(out.n_colours, c + 1);
    }
    out.colour_ptr.assign(size_t(out.n_colours) + 1, 0);
    for (int32_t v = 0; v < n; ++v) out.colour_ptr[size_t(out.colour[size_t(v)]) + 1]++;
    for (int32_t c = 0; c < out.n_colours; ++c) {
        out.max_class = std::max(out.max_class, out.colour_ptr[size_t(c) + 1]);
        out.colour_ptr[size_t(c) + 1] += out.colour_ptr[size_t(c)];
    }

    // slots in (colour, node) order
    auto put_terms = [&](int32_t c, int32_t skip, int32_t* lo, int32_t* cnt, int64_t* skip_stride) {
        *lo = int32_t(out.terms.size());
        int64_t stride = 1;
        std::vector<GibbsTerm> rev;
        for (int32_t e = in_ptr[c + 1] - 1; e >= in_ptr[c]; --e) {   // last parent least significant
            const int32_t p = in_idx[e];
            if (p == skip) *skip_stride = stride;
            else rev.push_back(GibbsTerm{stride, p, 0});
            stride *= k[p];
        }
        out.terms.insert(out.terms.end(), rev.rbegin(), rev.rend());
        *cnt = int32_t(rev.size());
    };
    out.slots.resize(size_t(n));
    std::vector<int32_t> fill(out.colour_ptr.begin(), out.colour_ptr.end());
    int64_t off = 0;
    std::vector<int32_t> hist_off(size_t(n), 0);
    for (int32_t v = 0; v < n; ++v) { hist_off[size_t(v)] = int32_t(off); off += k[v]; }
    for (int32_t v = 0; v < n; ++v) {
        GibbsSlot& s = out.slots[size_t(fill[size_t(out.colour[size_t(v)])]++)];
        s.cpt_off = cpt_off[v];
        s.node = v;
        s.k = k[v];
        s.hist_off = hist_off[size_t(v)];
        s.pad_ = 0;
        int64_t unused = 0;
        put_terms(v, -1, &s.term_lo, &s.term_n, &unused);
        s.child_lo = int32_t(out.children.size());
        s.child_n = int32_t(kids[size_t(v)].size());
        for (int32_t c : kids[size_t(v)]) {
            GibbsChild ch{};
            ch.cpt_off = cpt_off[c];
            ch.node = c;
            ch.k = k[c];
            ch.stride = 0;
            put_terms(c, v, &ch.term_lo, &ch.term_n, &ch.stride);
            out.children.push_back(ch);
        }
        out.reads_per_sweep += int64_t(k[v]) * (1 + int64_t(kids[size_t(v)].size()));
    }

    out.state_stride = (std::max(n, 1) + 15) & ~15;
    const int32_t hist_bytes = (out.cells * 4 + 15) & ~15;
    out.lanes_per_chain = kGibbsMinLanes;
    while (out.lanes_per_chain < 64 &&
           (out.lanes_per_chain < out.max_class || hist_bytes + (kGibbsThreads / out.lanes_per_chain) * out.state_stride > kGibbsLdsBudget))
        out.lanes_per_chain *= 2;
    out.chains_per_block = kGibbsThreads / out.lanes_per_chain;
    out.lds_bytes = hist_bytes + out.chains_per_block * out.state_stride;
    out.default_sweeps = int32_t(std::max<int64_t>(1, std::min<int64_t>(kGibbsDefaultSweeps, kGibbsLaunchReads / std::max<int64_t>(out.reads_per_sweep, 1))));
    out.ok = true;
}

std::vector<GibbsLaunch> gibbs_launches(uint64_t sweep_begin, uint64_t n_sweeps, int64_t cap) {
    std::vector<GibbsLaunch> out;
    for (uint64_t done = 0; done < n_sweeps; done += out.back().count) out.push_back(gibbs_launch_at(sweep_begin, n_sweeps, cap, done));
    return out;
}

uint64_t gibbs_kept_sweeps(uint64_t sweep_begin, uint64_t n_sweeps, uint64_t burn_in, uint64_t thin) {
    const uint64_t end = sweep_begin + n_sweeps, lo = std::max(sweep_begin, burn_in);
    if (thin == 0 || end <= lo) return 0;
    const uint64_t first = lo + (thin - (lo - burn_in) % thin) % thin;
    return first < end ? (end - 1 - first) / thin + 1 : 0;
}

}  // namespace bnmi
