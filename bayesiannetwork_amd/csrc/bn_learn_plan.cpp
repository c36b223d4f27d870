// bn_learn_plan.cpp -- the host-only planning of bn_learn_plan.hpp: checks, families, chunks, passes and launch order of a batch of
// family scores; the family table and lattice steps of a subset call.  Pure functions of the arities and the lists: no HIP call, no
// device state.  The error texts and the order of the checks are the C ABI's (include/bn_mi355x.h, bn_learn_score_groups / _subsets).
#include "bn_learn_plan.hpp"

#include <algorithm>
#include <utility>

#include "../../include/bn_mi355x.h"

namespace bnmi {
namespace {

using bn_eng::fail;

std::string gname(size_t g) { return "group " + std::to_string(g) + ": "; }

// the limits of one family: rows = product of the parents' arities
int check_family(const int32_t* k, size_t g, int32_t child, int64_t rows, int32_t n_parents) {
    if (n_parents > kLearnMaxParents)
        return fail(BN_ERR_ARG, gname(g) + "a family of " + std::to_string(n_parents) + " parents (at most " + std::to_string(kLearnMaxParents) + ")");
    if (rows * k[size_t(child)] > kLearnMaxEntries)
        return fail(BN_ERR_ARG, gname(g) + "a family table of more than 2^20 entries");
    return BN_OK;
}

int check_group(const int32_t* k, int32_t n, size_t g, const GroupIn& in, int64_t& base_rows) {
    if (in.child < 0 || in.child >= n) return fail(BN_ERR_ARG, gname(g) + "child id " + std::to_string(in.child) + " out of range");
    if (in.n_base < 0 || in.n_cand < 0 || (in.n_base > 0 && !in.base) || (in.n_cand > 0 && !in.cand))
        return fail(BN_ERR_ARG, gname(g) + "bad parent or candidate list");
    if (in.n_base > kLearnMaxParents)
        return fail(BN_ERR_ARG, gname(g) + "a family of " + std::to_string(in.n_base) + " parents (at most " + std::to_string(kLearnMaxParents) + ")");
    base_rows = 1;
    for (int32_t j = 0; j < in.n_base; ++j) {
        const int32_t u = in.base[j];
        if (u < 0 || u >= n) return fail(BN_ERR_ARG, gname(g) + "parent id " + std::to_string(u) + " out of range");
        if (u == in.child) return fail(BN_ERR_ARG, gname(g) + "the child is among its parents");
        if (j > 0 && u <= in.base[j - 1]) return fail(BN_ERR_ARG, gname(g) + "base parents must be strictly increasing");
        base_rows *= k[size_t(u)];   // (<= 255^16 < 2^63)
        if (base_rows > kLearnMaxEntries) break;
    }
    if (int r = check_family(k, g, in.child, base_rows, in.n_base)) return r;
    for (int32_t j = 0; j < in.n_cand; ++j) {
        const int32_t u = in.cand[j];
        if (u < 0 || u >= n) return fail(BN_ERR_ARG, gname(g) + "candidate id " + std::to_string(u) + " out of range");
        if (u == in.child) return fail(BN_ERR_ARG, gname(g) + "the child is among its candidates");
        if (std::binary_search(in.base, in.base + in.n_base, u))
            return fail(BN_ERR_ARG, gname(g) + "candidate " + std::to_string(u) + " is already a base parent");
        for (int32_t i = 0; i < j; ++i)
            if (in.cand[i] == u) return fail(BN_ERR_ARG, gname(g) + "candidate " + std::to_string(u) + " listed twice");
        if (int r = check_family(k, g, in.child, base_rows * k[size_t(u)], in.n_base + 1)) return r;
    }
    return BN_OK;
}

}  // namespace

int plan_groups(const int32_t* k, int32_t n, const std::vector<GroupIn>& groups, int64_t max_scratch_cells, GroupPlan& out) {
    out = GroupPlan{};
    std::vector<LearnChunk>& chunks = out.chunks;
    std::vector<LearnFamily> fams;   // in input order
    for (size_t g = 0; g < groups.size(); ++g) {
        const GroupIn& in = groups[g];
        int64_t base_rows = 1;
        if (int r = check_group(k, n, g, in, base_rows)) return r;
        const int32_t kc = k[size_t(in.child)];
        const int32_t base_at = int32_t(out.par_id.size());
        for (int32_t j = 0; j < in.n_base; ++j) {
            out.par_id.push_back(in.base[j]);
            out.par_k.push_back(k[size_t(in.base[j])]);
        }
        const int32_t fam_base = int32_t(fams.size());
        fams.push_back(LearnFamily{0, out.out_cells, int32_t(base_rows * kc), kc, 1, 1});
        out.out_cells += base_rows * kc;
        for (int32_t j = 0; j < in.n_cand; ++j) {
            const int32_t u = in.cand[j], ku = k[size_t(u)];
            int64_t low = 1;   // product of the arities of the base parents above u: where u's digit goes in the fitted layout
            for (int32_t i = in.n_base - 1; i >= 0 && in.base[i] > u; --i) low *= k[size_t(in.base[i])];
            fams.push_back(LearnFamily{0, out.out_cells, int32_t(base_rows * ku * kc), kc, ku, int32_t(low)});
            out.out_cells += base_rows * ku * kc;
        }
        // chunks: families that fit the LDS budget share blocks of <= kLearnLdsCells cells; the others go to device memory
        for (int lds = 1; lds >= 0; --lds) {
            bool open = false;
            for (int32_t j = -1; j < in.n_cand; ++j) {
                const int32_t fam = fam_base + 1 + j;
                const int32_t cells = fams[size_t(fam)].entries;
                if ((cells <= kLearnLdsCells) != (lds == 1)) continue;
                const int32_t cap_cand = lds ? kLearnMaxLdsCand : kLearnMaxGlobalCand;
                if (!open || chunks.back().n_cand >= cap_cand || (lds && chunks.back().cells + cells > kLearnLdsCells)) {
                    chunks.push_back(LearnChunk{0, in.child, kc, base_at, in.n_base, int32_t(out.cand_id.size()), 0, -1, 0, lds, 0});
                    out.base_fam.push_back(-1);
                    open = true;
                }
                LearnChunk& c = chunks.back();
                if (j < 0) {
                    c.base_cell = c.cells;
                    out.base_fam.back() = fam;
                } else {
                    out.cand_id.push_back(in.cand[j]);
                    out.cand_k.push_back(k[size_t(in.cand[j])]);
                    out.cand_cell.push_back(c.cells);
                    out.cand_fam.push_back(fam);
                    ++c.n_cand;
                }
                c.cells += cells;
            }
        }
    }
    const size_t n_fams = fams.size();
    if (n_fams == 0) return BN_OK;
    // passes: runs of whole chunks whose counter blocks fit the scratch; families follow their chunks, so a pass scores the
    // families of its chunks -- a group's families may therefore be scored by different passes, and are looked up by index
    std::vector<int32_t> fam_pass(n_fams, 0);
    {
        int64_t at = 0;
        int32_t first = 0;
        for (size_t c = 0; c < chunks.size(); ++c) {
            if (at > 0 && at + chunks[c].cells > max_scratch_cells) {
                out.passes.push_back(LearnPass{first, int32_t(c) - first, 0, 0, at});
                first = int32_t(c);
                at = 0;
            }
            chunks[c].count_at = at;
            const int32_t pass = int32_t(out.passes.size());
            if (out.base_fam[c] >= 0) {
                fams[size_t(out.base_fam[c])].count_at = at + chunks[c].base_cell;
                fam_pass[size_t(out.base_fam[c])] = pass;
            }
            for (int32_t j = 0; j < chunks[c].n_cand; ++j) {
                const int32_t fam = out.cand_fam[size_t(chunks[c].cand_at + j)];
                fams[size_t(fam)].count_at = at + out.cand_cell[size_t(chunks[c].cand_at + j)];
                fam_pass[size_t(fam)] = pass;
            }
            at += chunks[c].cells;
        }
        out.passes.push_back(LearnPass{first, int32_t(chunks.size()) - first, 0, 0, at});
    }
    // the scoring kernel takes a run of families: order them by pass (stable), and remember where each went
    out.order.resize(n_fams);
    for (size_t f = 0; f < n_fams; ++f) out.order[f] = int32_t(f);
    if (out.passes.size() > 1)
        std::stable_sort(out.order.begin(), out.order.end(), [&](int32_t x, int32_t y) { return fam_pass[size_t(x)] < fam_pass[size_t(y)]; });
    out.fams.resize(n_fams);
    for (size_t i = 0; i < n_fams; ++i) out.fams[i] = fams[size_t(out.order[i])];
    size_t fam_end = 0;
    for (size_t p = 0; p < out.passes.size(); ++p) {
        out.passes[p].fam0 = int32_t(fam_end);
        while (fam_end < n_fams && fam_pass[size_t(out.order[fam_end])] == int32_t(p)) ++fam_end;
        out.passes[p].n_fams = int32_t(fam_end) - out.passes[p].fam0;
        out.scratch_cells = std::max(out.scratch_cells, out.passes[p].cells);
    }
    return BN_OK;
}

// ---- the subset lattice: base + every subset of the candidates, from ONE count of the top family (bn_learn_lattice.hip) ----------

int plan_subsets(const int32_t* k, int32_t n, int32_t child, int32_t n_base, const int32_t* base, int32_t m, const int32_t* cand,
                 int64_t max_scratch_cells, SubsetPlan& sh) {
    sh = SubsetPlan{};
    if (child < 0 || child >= n) return fail(BN_ERR_ARG, "subsets: child id " + std::to_string(child) + " out of range");
    if (n_base < 0 || m < 0 || (n_base > 0 && !base) || (m > 0 && !cand)) return fail(BN_ERR_ARG, "subsets: bad parent or candidate list");
    if (int64_t(n_base) + m > kLearnMaxParents)
        return fail(BN_ERR_ARG, "subsets: the top family has " + std::to_string(int64_t(n_base) + m) + " parents (n_base + m at most " +
                                    std::to_string(kLearnMaxParents) + ")");
    std::vector<std::pair<int32_t, int32_t>> vars;
    for (int32_t j = 0; j < n_base + m; ++j) {
        const int32_t u = j < n_base ? base[j] : cand[j - n_base];
        const char* what = j < n_base ? "parent" : "candidate";
        if (u < 0 || u >= n) return fail(BN_ERR_ARG, std::string("subsets: ") + what + " id " + std::to_string(u) + " out of range");
        if (u == child) return fail(BN_ERR_ARG, std::string("subsets: the child is among its ") + what + "s");
        for (const auto& v : vars)
            if (v.first == u) return fail(BN_ERR_ARG, std::string("subsets: ") + what + " " + std::to_string(u) + " listed twice");
        vars.emplace_back(u, j < n_base ? -1 : j - n_base);
    }
    std::sort(vars.begin(), vars.end());
    sh.kc = k[size_t(child)];
    sh.top_cells = sh.kc;
    sh.all_cells = sh.kc;
    for (const auto& v : vars) {
        const int64_t ku = k[size_t(v.first)];
        sh.id.push_back(v.first);
        sh.k.push_back(int32_t(ku));
        sh.bit.push_back(v.second);
        sh.top_cells *= ku;                               // (<= 2^20 * 255 before the check below)
        sh.all_cells *= v.second < 0 ? ku : ku + 1;       // (<= 2^20 * 2^16 once the top family has passed)
        if (sh.top_cells > kLearnMaxEntries)
            return fail(BN_ERR_ARG, "subsets: the top family's table has more than 2^20 (" + std::to_string(kLearnMaxEntries) + ") entries");
    }
    if (sh.all_cells > max_scratch_cells)
        return fail(BN_ERR_ARG, "subsets: the 2^" + std::to_string(m) + " count tables need " + std::to_string(sh.all_cells) + " cells (at most 2^25 = " +
                                    std::to_string(max_scratch_cells) + " in the single pass)");
    const int32_t nv = n_base + m, n_fams = int32_t(1) << m, full = n_fams - 1;
    sh.nv = nv;
    sh.n_fams = n_fams;
    std::vector<LearnFamily>& fams = sh.fams;
    fams.resize(size_t(n_fams));
    {
        int64_t at = 0;
        for (int32_t mask = 0; mask < n_fams; ++mask) {
            int64_t cells = sh.kc;
            for (int32_t p = 0; p < nv; ++p)
                if (sh.bit[size_t(p)] < 0 || ((mask >> sh.bit[size_t(p)]) & 1)) cells *= sh.k[size_t(p)];
            fams[size_t(mask)] = LearnFamily{at, at, int32_t(cells), sh.kc, 1, 1};
            at += cells;
        }
    }
    sh.lds = sh.top_cells <= kLearnLdsCells;
    // the per-level form: family `mask` from mask + x, x the absent candidate with the smallest id (the longest contiguous runs)
    sh.level_at.assign(size_t(m) + 2, 0);
    sh.level_max.assign(size_t(m) + 1, 0);
    if (!sh.lds) {
        std::vector<std::vector<LatticeStep>> by_level(size_t(m) + 1);
        for (int32_t mask = 0; mask < full; ++mask) {
            int32_t px = -1, absent = 0;
            for (int32_t p = 0; p < nv; ++p)
                if (sh.bit[size_t(p)] >= 0 && !((mask >> sh.bit[size_t(p)]) & 1)) {
                    if (px < 0) px = p;
                    ++absent;
                }
            int64_t inner = sh.kc;
            for (int32_t p = px + 1; p < nv; ++p)
                if (sh.bit[size_t(p)] < 0 || ((mask >> sh.bit[size_t(p)]) & 1)) inner *= sh.k[size_t(p)];
            const int32_t sup = mask | (int32_t(1) << sh.bit[size_t(px)]);
            by_level[size_t(absent)].push_back(LatticeStep{fams[size_t(sup)].count_at, fams[size_t(mask)].count_at, fams[size_t(mask)].entries,
                                                           int32_t(inner), sh.k[size_t(px)], 0});
            sh.level_max[size_t(absent)] = std::max(sh.level_max[size_t(absent)], fams[size_t(mask)].entries);
        }
        for (int32_t l = 1; l <= m; ++l) {
            sh.level_at[size_t(l)] = int32_t(sh.steps.size());
            sh.steps.insert(sh.steps.end(), by_level[size_t(l)].begin(), by_level[size_t(l)].end());
        }
        sh.level_at[size_t(m) + 1] = int32_t(sh.steps.size());
    }
    sh.chunks.assign(1, LearnChunk{fams[size_t(full)].count_at, child, sh.kc, 0, nv, 0, 0, 0, int32_t(sh.top_cells), sh.lds ? 1 : 0, 0});
    return BN_OK;
}

}  // namespace bnmi
