// bn_learn.cpp -- C ABI of structure learning (include/bn_mi355x.h, bn_learn_*), reference bayesian/learning/greedy.hpp and
// k2_algorithm.hpp.  Kernels: bn_learn_kernels.hip.  bn_learn_score_groups scores batches of candidate families of a child against a
// device-resident pattern table; bn_learner holds a graph, every node's family term and the score, and bn_learn_try_parents is the
// reference's inner loop for one child with one device pass per ACCEPTED edge (plus one) instead of one fit and one score of the whole
// graph per candidate.  The logarithm is the device's fp64 log: the learner's score is its own stated function of the counts.
// bn_learn_score_subsets scores EVERY subset of a candidate parent set from one count of the top family (bn_learn_lattice.hip);
// bn_learn_best_parents, bn_learn_brute_force_hint and bn_learn_brute_force are the reference's bayesian/learning/brute_force.hpp on it.
// bn_term_table holds the family term of EVERY parent set of at most q nodes per child, made by one batch of run_groups;
// bn_learn_anneal runs the reference's simulated_annealing.hpp as many device-resident chains over it (bn_learn_anneal.hip).
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>

#include "bn_engine_internal.hpp"
#include "bn_info_table.hpp"
#include "bn_learn.hpp"
#include "bn_learn_anneal.hpp"
#include "bn_learn_hc.hpp"
#include "../../include/bn_mi355x.h"

namespace {

struct GroupIn {
    int32_t child;
    const int32_t* base;
    int32_t n_base;
    const int32_t* cand;
    int32_t n_cand;
};

struct LearnTimes {
    double count_ns = 0.0, score_ns = 0.0;
    int64_t families = 0, passes = 0;
    int64_t count_bytes = 0;   // what the counting kernel has to read, from the shapes: per chunk P * (8 + base + 1 + candidates)
    double lattice_ns = 0.0;   // the subset lattice's kernel(s)
    int64_t subsets = 0;       // families made by the lattice (the top family included)
    double anneal_ns = 0.0;    // the annealing kernel
    int64_t anneal_chains = 0, anneal_steps = 0;
    double hc_ns = 0.0;        // the hierarchical-clustering kernel
    int64_t hc_runs = 0, hc_merges = 0;
};

std::string gname(size_t g) { return "group " + std::to_string(g) + ": "; }

// The family term: kind 0 the log-likelihood term (AIC / MDL), 2 BDeu, 3 K2.  Held normalised (ess 0.0 where the kind does not
// read it), so two specs are the same function iff kind and the bits of ess agree.
const bn_score_spec kLogLikSpec{0, 0, 0.0};

int check_spec(const bn_score_spec* in, bn_score_spec& out) {
    out = kLogLikSpec;
    if (!in) return BN_OK;
    if (in->kind != 0 && in->kind != 2 && in->kind != 3)
        return fail(BN_ERR_ARG, "score spec: unknown kind " + std::to_string(in->kind) + " (0 log-likelihood term, 2 BDeu, 3 K2)");
    out.kind = in->kind;
    if (in->kind == 2) {
        if (!(std::isfinite(in->ess) && in->ess >= 0x1p-20 && in->ess <= 0x1p20))
            return fail(BN_ERR_ARG, "score spec: BDeu's ess must be finite and within [2^-20, 2^20]");
        out.ess = in->ess;
    }
    return BN_OK;
}

bool same_spec(const bn_score_spec& x, const bn_score_spec& y) { return x.kind == y.kind && std::memcmp(&x.ess, &y.ess, 8) == 0; }

const char* spec_name(const bn_score_spec& x) { return x.kind == 0 ? "the log-likelihood term (AIC / MDL)" : x.kind == 2 ? "BDeu" : "K2"; }

int launch_score(const bn_score_spec& spec, const LearnArgs& a, int32_t fam0, int32_t n_fams, void* stream) {
    return spec.kind == 0 ? learn_launch_score(a, fam0, n_fams, stream) : learn_launch_score_bd(a, fam0, n_fams, spec.kind, spec.ess, stream);
}

// the limits of one family: rows = product of the parents' arities
int check_family(const bn_info_table* t, size_t g, int32_t child, int64_t rows, int32_t n_parents) {
    if (n_parents > kLearnMaxParents)
        return fail(BN_ERR_ARG, gname(g) + "a family of " + std::to_string(n_parents) + " parents (at most " + std::to_string(kLearnMaxParents) + ")");
    if (rows * t->k[size_t(child)] > kLearnMaxEntries)
        return fail(BN_ERR_ARG, gname(g) + "a family table of more than 2^20 entries");
    return BN_OK;
}

int check_group(const bn_info_table* t, size_t g, const GroupIn& in, int64_t& base_rows) {
    const int32_t n = t->n;
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
        base_rows *= t->k[size_t(u)];   // (<= 255^16 < 2^63)
        if (base_rows > kLearnMaxEntries) break;
    }
    if (int r = check_family(t, g, in.child, base_rows, in.n_base)) return r;
    for (int32_t j = 0; j < in.n_cand; ++j) {
        const int32_t u = in.cand[j];
        if (u < 0 || u >= n) return fail(BN_ERR_ARG, gname(g) + "candidate id " + std::to_string(u) + " out of range");
        if (u == in.child) return fail(BN_ERR_ARG, gname(g) + "the child is among its candidates");
        if (std::binary_search(in.base, in.base + in.n_base, u))
            return fail(BN_ERR_ARG, gname(g) + "candidate " + std::to_string(u) + " is already a base parent");
        for (int32_t i = 0; i < j; ++i)
            if (in.cand[i] == u) return fail(BN_ERR_ARG, gname(g) + "candidate " + std::to_string(u) + " listed twice");
        if (int r = check_family(t, g, in.child, base_rows * t->k[size_t(u)], in.n_base + 1)) return r;
    }
    return BN_OK;
}

// ll_out [families], group-major, base first; counts_out: null, or every family's counts back to back in the fitted layout
int run_groups(bn_info_table* t, const bn_score_spec& spec, const std::vector<GroupIn>& groups, double* ll_out, uint64_t* counts_out,
               LearnTimes* times) {
    std::vector<LearnChunk> chunks;
    std::vector<LearnFamily> fams;
    std::vector<int32_t> par_id, par_k, cand_id, cand_k, cand_cell;
    std::vector<int32_t> cand_fam;   // family of every chunk candidate
    std::vector<int32_t> chunk_base_fam;   // family of the chunk's base, or -1
    int64_t out_cells = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        const GroupIn& in = groups[g];
        int64_t base_rows = 1;
        if (int r = check_group(t, g, in, base_rows)) return r;
        const int32_t kc = t->k[size_t(in.child)];
        const int32_t base_at = int32_t(par_id.size());
        for (int32_t j = 0; j < in.n_base; ++j) {
            par_id.push_back(in.base[j]);
            par_k.push_back(t->k[size_t(in.base[j])]);
        }
        const int32_t fam_base = int32_t(fams.size());
        fams.push_back(LearnFamily{0, out_cells, int32_t(base_rows * kc), kc, 1, 1});
        out_cells += base_rows * kc;
        for (int32_t j = 0; j < in.n_cand; ++j) {
            const int32_t u = in.cand[j], ku = t->k[size_t(u)];
            int64_t low = 1;   // product of the arities of the base parents above u: where u's digit goes in the fitted layout
            for (int32_t i = in.n_base - 1; i >= 0 && in.base[i] > u; --i) low *= t->k[size_t(in.base[i])];
            fams.push_back(LearnFamily{0, out_cells, int32_t(base_rows * ku * kc), kc, ku, int32_t(low)});
            out_cells += base_rows * ku * kc;
        }
        // chunks: families that fit the LDS budget share blocks of <= kLearnLdsCells cells; the others go to device memory
        auto open_chunk = [&](bool lds) {
            chunks.push_back(LearnChunk{0, in.child, kc, base_at, in.n_base, int32_t(cand_id.size()), 0, -1, 0, lds ? 1 : 0, 0});
            chunk_base_fam.push_back(-1);
        };
        for (int lds = 1; lds >= 0; --lds) {
            bool open = false;
            for (int32_t j = -1; j < in.n_cand; ++j) {
                const int32_t fam = fam_base + 1 + j;
                const int32_t cells = fams[size_t(fam)].entries;
                if ((cells <= kLearnLdsCells) != (lds == 1)) continue;
                const int32_t cap_cand = lds ? kLearnMaxLdsCand : kLearnMaxGlobalCand;
                if (!open || chunks.back().n_cand >= cap_cand || (lds && chunks.back().cells + cells > kLearnLdsCells)) {
                    open_chunk(lds == 1);
                    open = true;
                }
                LearnChunk& c = chunks.back();
                if (j < 0) {
                    c.base_cell = c.cells;
                    chunk_base_fam.back() = fam;
                } else {
                    cand_id.push_back(in.cand[j]);
                    cand_k.push_back(t->k[size_t(in.cand[j])]);
                    cand_cell.push_back(c.cells);
                    cand_fam.push_back(fam);
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
    struct Pass { int32_t chunk0, chunk1; int64_t cells; };
    std::vector<Pass> passes;
    std::vector<int32_t> fam_pass(n_fams, 0);
    {
        int64_t at = 0;
        int32_t first = 0;
        for (size_t c = 0; c < chunks.size(); ++c) {
            if (at > 0 && at + chunks[c].cells > kLearnMaxScratchCells) {
                passes.push_back(Pass{first, int32_t(c), at});
                first = int32_t(c);
                at = 0;
            }
            chunks[c].count_at = at;
            const int32_t pass = int32_t(passes.size());
            if (chunk_base_fam[c] >= 0) {
                fams[size_t(chunk_base_fam[c])].count_at = at + chunks[c].base_cell;
                fam_pass[size_t(chunk_base_fam[c])] = pass;
            }
            for (int32_t j = 0; j < chunks[c].n_cand; ++j) {
                const int32_t fam = cand_fam[size_t(chunks[c].cand_at + j)];
                fams[size_t(fam)].count_at = at + cand_cell[size_t(chunks[c].cand_at + j)];
                fam_pass[size_t(fam)] = pass;
            }
            at += chunks[c].cells;
        }
        passes.push_back(Pass{first, int32_t(chunks.size()), at});
    }
    // the scoring kernel takes a run of families: order them by pass (stable), and remember where each went
    std::vector<int32_t> order(n_fams);
    for (size_t f = 0; f < n_fams; ++f) order[f] = int32_t(f);
    if (passes.size() > 1) std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return fam_pass[size_t(x)] < fam_pass[size_t(y)]; });
    std::vector<LearnFamily> fams_sorted(n_fams);
    for (size_t i = 0; i < n_fams; ++i) fams_sorted[i] = fams[size_t(order[i])];

    ON_DEVICE(t);
    hipStream_t s = t->stream;
    int64_t scratch = 0;
    for (const Pass& p : passes) scratch = std::max(scratch, p.cells);
    DeviceBuf<LearnChunk> d_chunks;
    DeviceBuf<LearnFamily> d_fams;
    DeviceBuf<int32_t> d_par_id, d_par_k, d_cand_id, d_cand_k, d_cand_cell;
    DeviceBuf<unsigned long long> d_N, d_out;
    DeviceBuf<double> d_ll;
    EventOwner ev0, ev1, ev2;
    int r;
    if ((r = upload(d_chunks, chunks, s)) || (r = upload(d_fams, fams_sorted, s)) || (r = upload(d_par_id, par_id, s)) ||
        (r = upload(d_par_k, par_k, s)) || (r = upload(d_cand_id, cand_id, s)) || (r = upload(d_cand_k, cand_k, s)) ||
        (r = upload(d_cand_cell, cand_cell, s)) || (r = dalloc(d_N, size_t(scratch))) || (r = dalloc(d_ll, n_fams)))
        return r;
    if (counts_out && (r = dalloc(d_out, size_t(out_cells)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HIPCHK(hipEventCreate(ev2.put()));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus <= 0) cus = 256;
    int forced = 0;
    if (const char* env = std::getenv("BN_LEARN_SPLITS")) forced = std::atoi(env);
    const LearnArgs a{t->d_T, t->d_w, t->P, t->Ppad, d_chunks, d_par_id, d_par_k, d_cand_id, d_cand_k, d_cand_cell, d_N, d_fams, d_ll,
                      counts_out ? d_out.get() : nullptr};
    size_t fam_at = 0;
    double call_count_ns = 0.0, call_score_ns = 0.0;
    for (size_t pi = 0; pi < passes.size(); ++pi) {
        const Pass& p = passes[pi];
        const int32_t n_chunks = p.chunk1 - p.chunk0;
        size_t fam_end = fam_at;
        while (fam_end < n_fams && fam_pass[size_t(order[fam_end])] == int32_t(pi)) ++fam_end;
        // a short batch leaves a long table to a handful of CUs: split the patterns until about four workgroups per CU exist,
        // each keeping at least two tiles (bn_score_nodes' rule)
        int splits = forced;
        if (splits <= 0) {
            const int64_t by_chip = (int64_t(4) * cus + n_chunks - 1) / std::max(n_chunks, 1);
            const int64_t by_work = (t->P + 2 * kLearnTile - 1) / (2 * kLearnTile);
            splits = int(std::min(by_chip, by_work));
        }
        splits = std::max(1, std::min(splits, 65535));
        HIPCHK(hipEventRecord(ev0, s));
        HIPCHK(hipMemsetAsync(d_N, 0, size_t(std::max<int64_t>(p.cells, 1)) * 8, s));
        if (int err = learn_launch_count(a, p.chunk0, n_chunks, splits, s))
            return fail(BN_ERR_HIP, std::string("family-group count kernel: ") + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev1, s));
        if (int err = launch_score(spec, a, int32_t(fam_at), int32_t(fam_end - fam_at), s))
            return fail(BN_ERR_HIP, std::string("family score kernel: ") + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev2, s));
        HIPCHK(hipStreamSynchronize(s));
        {
            float ms_count = 0.0f, ms_score = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms_count, ev0, ev1));
            HIPCHK(hipEventElapsedTime(&ms_score, ev1, ev2));
            call_count_ns += double(ms_count) * 1e6;
            call_score_ns += double(ms_score) * 1e6;
        }
        fam_at = fam_end;
    }
    std::vector<double> ll(n_fams);
    HIPCHK(hipMemcpyAsync(ll.data(), d_ll, n_fams * 8, hipMemcpyDeviceToHost, s));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, d_out, size_t(out_cells) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n_fams; ++i) ll_out[size_t(order[i])] = ll[i];
    t->learn_count_ns = call_count_ns;
    t->learn_lattice_ns = 0.0;
    t->learn_score_ns = call_score_ns;
    if (times) {
        times->count_ns += call_count_ns;
        times->score_ns += call_score_ns;
        times->families += int64_t(n_fams);
        times->passes += 1;
        for (const LearnChunk& c : chunks) times->count_bytes += t->P * int64_t(8 + c.n_base + 1 + c.n_cand);
    }
    return BN_OK;
}

// ---- the subset lattice: base + every subset of the candidates, from ONE count of the top family (bn_learn_lattice.hip) ----------

struct SubsetShape {
    std::vector<int32_t> id, k, bit;   // the top family's variables in increasing id; bit: the candidate's index, -1 for a base parent
    int32_t kc = 1;
    int64_t top_cells = 0, all_cells = 0;
};

int check_subsets(const bn_info_table* t, int32_t child, int32_t n_base, const int32_t* base, int32_t m, const int32_t* cand, SubsetShape& sh) {
    const int32_t n = t->n;
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
    sh.kc = t->k[size_t(child)];
    sh.top_cells = sh.kc;
    sh.all_cells = sh.kc;
    for (const auto& v : vars) {
        const int64_t ku = t->k[size_t(v.first)];
        sh.id.push_back(v.first);
        sh.k.push_back(int32_t(ku));
        sh.bit.push_back(v.second);
        sh.top_cells *= ku;                               // (<= 2^20 * 255 before the check below)
        sh.all_cells *= v.second < 0 ? ku : ku + 1;       // (<= 2^20 * 2^16 once the top family has passed)
        if (sh.top_cells > kLearnMaxEntries)
            return fail(BN_ERR_ARG, "subsets: the top family's table has more than 2^20 (" + std::to_string(kLearnMaxEntries) + ") entries");
    }
    if (sh.all_cells > kLearnMaxScratchCells)
        return fail(BN_ERR_ARG, "subsets: the 2^" + std::to_string(m) + " count tables need " + std::to_string(sh.all_cells) + " cells (at most 2^25 = " +
                                    std::to_string(kLearnMaxScratchCells) + " in the single pass)");
    return BN_OK;
}

// ll_out [2^m] in mask order (bit j: cand[j] is a parent); counts_out: null, or every family's counts in the fitted layout, mask order
int run_subsets(bn_info_table* t, const bn_score_spec& spec, int32_t child, int32_t n_base, const int32_t* base, int32_t m, const int32_t* cand,
                double* ll_out, uint64_t* counts_out, LearnTimes* times) {
    SubsetShape sh;
    if (int r = check_subsets(t, child, n_base, base, m, cand, sh)) return r;
    const int32_t nv = n_base + m, n_fams = int32_t(1) << m, full = n_fams - 1;
    std::vector<LearnFamily> fams(static_cast<size_t>(n_fams));
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
    const bool lds = sh.top_cells <= kLearnLdsCells;
    // the per-level form: family `mask` from mask + x, x the absent candidate with the smallest id (the longest contiguous runs)
    std::vector<LatticeStep> steps;
    std::vector<int32_t> level_at(size_t(m) + 2, 0), level_max(size_t(m) + 1, 0);
    if (!lds) {
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
            level_max[size_t(absent)] = std::max(level_max[size_t(absent)], fams[size_t(mask)].entries);
        }
        for (int32_t l = 1; l <= m; ++l) {
            level_at[size_t(l)] = int32_t(steps.size());
            steps.insert(steps.end(), by_level[size_t(l)].begin(), by_level[size_t(l)].end());
        }
        level_at[size_t(m) + 1] = int32_t(steps.size());
    }
    const std::vector<LearnChunk> chunks{LearnChunk{fams[size_t(full)].count_at, child, sh.kc, 0, nv, 0, 0, 0, int32_t(sh.top_cells), lds ? 1 : 0, 0}};

    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<LearnChunk> d_chunks;
    DeviceBuf<LearnFamily> d_fams;
    DeviceBuf<LatticeStep> d_steps;
    DeviceBuf<int32_t> d_par_id, d_par_k;
    DeviceBuf<unsigned long long> d_N, d_out;
    DeviceBuf<double> d_ll;
    EventOwner ev0, ev1, ev2, ev3;
    int r;
    if ((r = upload(d_chunks, chunks, s)) || (r = upload(d_fams, fams, s)) || (r = upload(d_steps, steps, s)) || (r = upload(d_par_id, sh.id, s)) ||
        (r = upload(d_par_k, sh.k, s)) || (r = dalloc(d_N, size_t(sh.all_cells))) || (r = dalloc(d_ll, size_t(n_fams))))
        return r;
    if (counts_out && (r = dalloc(d_out, size_t(sh.all_cells)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HIPCHK(hipEventCreate(ev2.put()));
    HIPCHK(hipEventCreate(ev3.put()));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus <= 0) cus = 256;
    int splits = 0;
    if (const char* env = std::getenv("BN_LEARN_SPLITS")) splits = std::atoi(env);
    if (splits <= 0) splits = int(std::min<int64_t>(int64_t(4) * cus, (t->P + 2 * kLearnTile - 1) / (2 * kLearnTile)));   // (run_groups' rule, one chunk)
    splits = std::max(1, std::min(splits, 65535));
    const LearnArgs a{t->d_T, t->d_w, t->P, t->Ppad, d_chunks, d_par_id, d_par_k, nullptr, nullptr, nullptr, d_N, d_fams, d_ll,
                      counts_out ? d_out.get() : nullptr};
    HIPCHK(hipEventRecord(ev0, s));
    HIPCHK(hipMemsetAsync(d_N.get() + fams[size_t(full)].count_at, 0, size_t(sh.top_cells) * 8, s));   // (the lattice writes every other cell)
    if (int err = learn_launch_count(a, 0, 1, splits, s))
        return fail(BN_ERR_HIP, std::string("top-family count kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    if (lds) {
        LatticeLds la{d_N, d_fams, n_fams, nv, int32_t(sh.top_cells), 0, {}, {}};
        for (int32_t p = 0; p < nv; ++p) {
            la.k[p] = sh.k[size_t(p)];
            la.bit[p] = sh.bit[size_t(p)];
        }
        // 56 KiB of LDS per workgroup: two per CU
        if (int err = learn_launch_lattice_lds(la, std::min(full, 2 * cus), s))
            return fail(BN_ERR_HIP, std::string("subset lattice kernel: ") + hipGetErrorString(hipError_t(err)));
    } else {
        for (int32_t l = 1; l <= m; ++l)
            if (int err = learn_launch_lattice_level(d_N, d_steps, level_at[size_t(l)], level_at[size_t(l) + 1] - level_at[size_t(l)],
                                                     level_max[size_t(l)], s))
                return fail(BN_ERR_HIP, std::string("subset lattice level kernel: ") + hipGetErrorString(hipError_t(err)));
    }
    HIPCHK(hipEventRecord(ev2, s));
    if (int err = launch_score(spec, a, 0, n_fams, s))
        return fail(BN_ERR_HIP, std::string("family score kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev3, s));
    HIPCHK(hipMemcpyAsync(ll_out, d_ll, size_t(n_fams) * 8, hipMemcpyDeviceToHost, s));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, d_out, size_t(sh.all_cells) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms_count = 0.0f, ms_lattice = 0.0f, ms_score = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms_count, ev0, ev1));
    HIPCHK(hipEventElapsedTime(&ms_lattice, ev1, ev2));
    HIPCHK(hipEventElapsedTime(&ms_score, ev2, ev3));
    t->learn_count_ns = double(ms_count) * 1e6;
    t->learn_lattice_ns = double(ms_lattice) * 1e6;
    t->learn_score_ns = double(ms_score) * 1e6;
    if (times) {
        times->count_ns += t->learn_count_ns;
        times->lattice_ns += t->learn_lattice_ns;
        times->score_ns += t->learn_score_ns;
        times->families += n_fams;
        times->subsets += n_fams;
        times->passes += 1;
        times->count_bytes += t->P * int64_t(8 + nv + 1);
    }
    return BN_OK;
}

}  // namespace

struct bn_learner {
    bn_info_table* t = nullptr;
    int32_t n = 0, criterion = 0, max_parents = 0;
    std::vector<std::vector<int32_t>> parents, children;   // parents increasing per node
    std::vector<double> ll;                                // family term of every node
    int64_t params = 0;
    double penalty = 1.0;    // per parameter: 1 (AIC), log2(total) / 2 (MDL); criteria 2 (BDeu) and 3 (K2) have none
    double score = 0.0;
    bn_score_spec spec = kLogLikSpec;   // the family term: kind 0 under AIC / MDL, else the criterion
    LearnTimes times;

    int64_t family_params(int32_t v, int64_t rows) const { return int64_t(t->k[size_t(v)] - 1) * rows; }
    int64_t rows_of(int32_t v) const {
        int64_t rows = 1;
        for (int32_t u : parents[size_t(v)]) rows *= t->k[size_t(u)];
        return rows;
    }
    // evaluation.py's arithmetic: likelihood = 0.0; likelihood -= ll[v] in node order; + double(params) * penalty
    double score_with(int32_t c, double ll_c, int64_t params_now) const {
        double likelihood = 0.0;
        for (int32_t v = 0; v < n; ++v) likelihood -= v == c ? ll_c : ll[size_t(v)];
        if (criterion >= 2) return likelihood;
        return criterion == 0 ? likelihood + double(params_now) : likelihood + double(params_now) * penalty;
    }
};

extern "C" int bn_learn_score_groups_spec(bn_info_table* t, const bn_score_spec* spec_in, int32_t n_groups, const int32_t* child,
                                          const int32_t* base_ptr, const int32_t* base_idx, const int32_t* cand_ptr, const int32_t* cand_idx,
                                          double* ll_out, uint64_t* counts_out) {
    if (!t || !ll_out) return fail(BN_ERR_ARG, "null argument");
    bn_score_spec spec;
    if (int r = check_spec(spec_in, spec)) return r;
    if (n_groups < 0) return fail(BN_ERR_ARG, "n_groups < 0");
    if (n_groups > 0 && (!child || !base_ptr || !cand_ptr)) return fail(BN_ERR_ARG, "null argument");
    std::vector<GroupIn> groups(static_cast<size_t>(n_groups));
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t b0 = base_ptr[g], b1 = base_ptr[g + 1], c0 = cand_ptr[g], c1 = cand_ptr[g + 1];
        if (b0 < 0 || b1 < b0 || c0 < 0 || c1 < c0 || (b1 > b0 && !base_idx) || (c1 > c0 && !cand_idx))
            return fail(BN_ERR_ARG, gname(size_t(g)) + "bad parent or candidate list");
        groups[size_t(g)] = GroupIn{child[g], base_idx ? base_idx + b0 : nullptr, b1 - b0, cand_idx ? cand_idx + c0 : nullptr, c1 - c0};
    }
    return run_groups(t, spec, groups, ll_out, counts_out, nullptr);
}

extern "C" int bn_learn_score_groups(bn_info_table* t, int32_t n_groups, const int32_t* child, const int32_t* base_ptr,
                                     const int32_t* base_idx, const int32_t* cand_ptr, const int32_t* cand_idx, double* ll_out,
                                     uint64_t* counts_out) {
    return bn_learn_score_groups_spec(t, nullptr, n_groups, child, base_ptr, base_idx, cand_ptr, cand_idx, ll_out, counts_out);
}

static int learn_create(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, const bn_score_spec& spec,
                        int32_t max_parents, bn_learner** out);

extern "C" int bn_learn_create(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, int32_t max_parents,
                               bn_learner** out) {
    if (!out) return fail(BN_ERR_ARG, "null argument");
    *out = nullptr;
    if (!t || !in_ptr) return fail(BN_ERR_ARG, "null argument");
    if (criterion != 0 && criterion != 1) return fail(BN_ERR_ARG, "criterion: 0 AIC, 1 MDL");
    return learn_create(t, in_ptr, in_idx, criterion, kLogLikSpec, max_parents, out);
}

extern "C" int bn_learn_create_spec(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, const bn_score_spec* spec_in,
                                    int32_t max_parents, bn_learner** out) {
    if (!out) return fail(BN_ERR_ARG, "null argument");
    *out = nullptr;
    if (criterion < 0 || criterion > 3) return fail(BN_ERR_ARG, "criterion: 0 AIC, 1 MDL, 2 BDeu, 3 K2");
    bn_score_spec spec;
    if (int r = check_spec(spec_in, spec)) return r;
    if (spec.kind != (criterion >= 2 ? criterion : 0))
        return fail(BN_ERR_ARG, "criterion " + std::to_string(criterion) + " takes a score spec of kind " + std::to_string(criterion >= 2 ? criterion : 0) +
                                    ", not " + std::to_string(spec.kind) + (criterion >= 2 && !spec_in ? " (no spec given)" : ""));
    return learn_create(t, in_ptr, in_idx, criterion, spec, max_parents, out);
}

static int learn_create(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, const bn_score_spec& spec,
                        int32_t max_parents, bn_learner** out) {
    if (!t || !in_ptr) return fail(BN_ERR_ARG, "null argument");
    if (max_parents < 0 || max_parents > kLearnMaxParents) return fail(BN_ERR_ARG, "max_parents must be in 0..16");
    const int32_t n = t->n;
    if (in_ptr[0] != 0) return fail(BN_ERR_ARG, "in_ptr must start at 0");
    for (int32_t v = 0; v < n; ++v)
        if (in_ptr[v + 1] < in_ptr[v]) return fail(BN_ERR_ARG, "in_ptr must not decrease");
    if (in_ptr[n] > 0 && !in_idx) return fail(BN_ERR_ARG, "null argument");
    std::unique_ptr<bn_learner> L(new (std::nothrow) bn_learner);
    if (!L) return fail(BN_ERR_ALLOC, "host allocation failed");
    L->t = t;
    L->n = n;
    L->criterion = criterion;
    L->spec = spec;
    L->max_parents = max_parents;
    L->penalty = criterion == 1 ? std::log2(t->Nd) / 2 : 1.0;
    L->parents.resize(size_t(n));
    L->children.resize(size_t(n));
    for (int32_t v = 0; v < n; ++v) {
        std::vector<int32_t>& p = L->parents[size_t(v)];
        p.assign(in_idx + in_ptr[v], in_idx + in_ptr[v + 1]);
        for (int32_t u : p)
            if (u < 0 || u >= n || u == v) return fail(BN_ERR_ARG, "node " + std::to_string(v) + ": parent id " + std::to_string(u) + " out of range or the node itself");
        std::sort(p.begin(), p.end());
        if (std::adjacent_find(p.begin(), p.end()) != p.end()) return fail(BN_ERR_ARG, "node " + std::to_string(v) + ": a parent listed twice");
        for (int32_t u : p) L->children[size_t(u)].push_back(v);
    }
    {   // acyclic: every node leaves a queue of nodes without unvisited parents
        std::vector<int32_t> left(static_cast<size_t>(n)), queue;
        for (int32_t v = 0; v < n; ++v)
            if ((left[size_t(v)] = int32_t(L->parents[size_t(v)].size())) == 0) queue.push_back(v);
        for (size_t i = 0; i < queue.size(); ++i)
            for (int32_t c : L->children[size_t(queue[i])])
                if (--left[size_t(c)] == 0) queue.push_back(c);
        if (int32_t(queue.size()) != n) return fail(BN_ERR_ARG, "the starting graph has a cycle");
    }
    std::vector<GroupIn> groups(static_cast<size_t>(n));
    for (int32_t v = 0; v < n; ++v) groups[size_t(v)] = GroupIn{v, L->parents[size_t(v)].data(), int32_t(L->parents[size_t(v)].size()), nullptr, 0};
    L->ll.assign(size_t(n), 0.0);
    if (int r = run_groups(t, spec, groups, L->ll.data(), nullptr, &L->times)) return r;   // (names the node as "group v" when over a limit)
    for (int32_t v = 0; v < n; ++v) L->params += L->family_params(v, L->rows_of(v));
    L->score = L->score_with(-1, 0.0, L->params);
    *out = L.release();
    return BN_OK;
}

extern "C" void bn_learn_destroy(bn_learner* L) { delete L; }

extern "C" int bn_learn_try_parents(bn_learner* L, int32_t child, int32_t n_cand, const int32_t* cand, uint8_t* accepted_out) {
    if (!L || n_cand < 0 || (n_cand > 0 && (!cand || !accepted_out))) return fail(BN_ERR_ARG, "null argument or n_cand < 0");
    const int32_t n = L->n;
    if (child < 0 || child >= n) return fail(BN_ERR_ARG, "child id " + std::to_string(child) + " out of range");
    for (int32_t i = 0; i < n_cand; ++i)
        if (cand[i] < 0 || cand[i] >= n) return fail(BN_ERR_ARG, "candidate id " + std::to_string(cand[i]) + " out of range");
    std::fill(accepted_out, accepted_out + n_cand, uint8_t(0));
    // what the child reaches (graph.hpp:270, is_able_trace(to, from)): an edge from there would close a cycle.  Edges INTO the
    // child add no path that starts at it, so the set holds for the whole call.
    std::vector<uint8_t> reached(size_t(n), 0);
    {
        std::vector<int32_t> stack{child};
        reached[size_t(child)] = 1;
        while (!stack.empty()) {
            const int32_t v = stack.back();
            stack.pop_back();
            for (int32_t c : L->children[size_t(v)])
                if (!reached[size_t(c)]) { reached[size_t(c)] = 1; stack.push_back(c); }
        }
    }
    std::vector<int32_t>& par = L->parents[size_t(child)];
    const int32_t kc = L->t->k[size_t(child)];
    std::vector<int32_t> fam_of(size_t(n), -1), uniq;
    std::vector<double> ll;
    int32_t pos = 0;
    while (pos < n_cand) {
        if (int32_t(par.size()) >= L->max_parents || int32_t(par.size()) >= kLearnMaxParents) break;
        const int64_t rows = L->rows_of(child);
        // the candidates still ahead that may be added at all, each once, in walking order
        uniq.clear();
        for (int32_t i = pos; i < n_cand; ++i) {
            const int32_t u = cand[i];
            if (reached[size_t(u)] || fam_of[size_t(u)] >= 0 || std::binary_search(par.begin(), par.end(), u)) continue;
            if (rows * L->t->k[size_t(u)] * kc > kLearnMaxEntries) continue;
            fam_of[size_t(u)] = int32_t(uniq.size()) + 1;
            uniq.push_back(u);
        }
        for (int32_t u : uniq) fam_of[size_t(u)] = -1;
        if (uniq.empty()) break;
        const std::vector<GroupIn> group{GroupIn{child, par.data(), int32_t(par.size()), uniq.data(), int32_t(uniq.size())}};
        ll.assign(uniq.size() + 1, 0.0);
        if (int r = run_groups(L->t, L->spec, group, ll.data(), nullptr, &L->times)) return r;
        for (size_t j = 0; j < uniq.size(); ++j) fam_of[size_t(uniq[j])] = int32_t(j) + 1;
        int32_t taken = -1;
        for (int32_t i = pos; i < n_cand && taken < 0; ++i) {
            const int32_t u = cand[i], f = fam_of[size_t(u)];
            if (f < 0) continue;
            const int64_t params_next = L->params - L->family_params(child, rows) + L->family_params(child, rows * L->t->k[size_t(u)]);
            const double score_next = L->score_with(child, ll[size_t(f)], params_next);
            if (score_next < L->score) {   // strict (greedy.hpp:47, k2_algorithm.hpp:54)
                taken = i;
                L->ll[size_t(child)] = ll[size_t(f)];
                L->params = params_next;
                L->score = score_next;
            }
        }
        for (int32_t u : uniq) fam_of[size_t(u)] = -1;
        if (taken < 0) break;
        const int32_t u = cand[taken];
        par.insert(std::lower_bound(par.begin(), par.end(), u), u);
        L->children[size_t(u)].push_back(child);
        accepted_out[taken] = 1;
        pos = taken + 1;
    }
    return BN_OK;
}

extern "C" int bn_learn_score(const bn_learner* L, double* score_out) {
    if (!L || !score_out) return fail(BN_ERR_ARG, "null argument");
    *score_out = L->score;
    return BN_OK;
}

extern "C" int bn_learn_structure(const bn_learner* L, int32_t* in_ptr_out, int32_t* in_idx_out) {
    if (!L || !in_ptr_out) return fail(BN_ERR_ARG, "null argument");
    int32_t at = 0;
    in_ptr_out[0] = 0;
    for (int32_t v = 0; v < L->n; ++v) {
        for (int32_t u : L->parents[size_t(v)]) {
            if (!in_idx_out) return fail(BN_ERR_ARG, "null argument");
            in_idx_out[at++] = u;
        }
        in_ptr_out[v + 1] = at;
    }
    return BN_OK;
}

extern "C" int bn_learn_get(const bn_learner* L, const char* name, int64_t* out) {
    if (!L || !name || !out) return fail(BN_ERR_ARG, "null argument");
    const std::string s(name);
    if (s == "families_scored") *out = L->times.families;
    else if (s == "passes") *out = L->times.passes;
    else if (s == "count_ns") *out = int64_t(L->times.count_ns);
    else if (s == "score_ns") *out = int64_t(L->times.score_ns);
    else if (s == "count_bytes") *out = L->times.count_bytes;
    else if (s == "lattice_ns") *out = int64_t(L->times.lattice_ns);
    else if (s == "subsets_scored") *out = L->times.subsets;
    else if (s == "anneal_ns") *out = int64_t(L->times.anneal_ns);
    else if (s == "anneal_chains") *out = L->times.anneal_chains;
    else if (s == "anneal_steps") *out = L->times.anneal_steps;
    else if (s == "hc_ns") *out = int64_t(L->times.hc_ns);
    else if (s == "hc_runs") *out = L->times.hc_runs;
    else if (s == "hc_merges") *out = L->times.hc_merges;
    else if (s == "edges") {
        *out = 0;
        for (const auto& p : L->parents) *out += int64_t(p.size());
    } else if (s == "parameters") *out = L->params;
    else if (s == "criterion") *out = L->criterion;
    else return fail(BN_ERR_ARG, "unknown name (criterion, families_scored, passes, count_ns, score_ns, count_bytes, lattice_ns, subsets_scored, anneal_ns, anneal_chains, anneal_steps, hc_ns, hc_runs, hc_merges, edges, parameters)");
    return BN_OK;
}

// ---- exhaustive search: the subset lattice per child (reference bayesian/learning/brute_force.hpp) ----------------------------------

extern "C" int bn_learn_score_subsets_spec(bn_info_table* t, const bn_score_spec* spec_in, int32_t child, int32_t n_base, const int32_t* base,
                                           int32_t m, const int32_t* cand, double* ll_out, uint64_t* counts_out) {
    if (!t || !ll_out) return fail(BN_ERR_ARG, "null argument");
    bn_score_spec spec;
    if (int r = check_spec(spec_in, spec)) return r;
    return run_subsets(t, spec, child, n_base, base, m, cand, ll_out, counts_out, nullptr);
}

extern "C" int bn_learn_score_subsets(bn_info_table* t, int32_t child, int32_t n_base, const int32_t* base, int32_t m, const int32_t* cand,
                                      double* ll_out, uint64_t* counts_out) {
    return bn_learn_score_subsets_spec(t, nullptr, child, n_base, base, m, cand, ll_out, counts_out);
}

namespace {

// every node with a path from `from` in the learner's graph, `from` included (graph.hpp:270, is_able_trace)
std::vector<uint8_t> reached_from(const bn_learner* L, int32_t from) {
    std::vector<uint8_t> reached(size_t(L->n), 0);
    std::vector<int32_t> stack{from};
    reached[size_t(from)] = 1;
    while (!stack.empty()) {
        const int32_t v = stack.back();
        stack.pop_back();
        for (int32_t c : L->children[size_t(v)])
            if (!reached[size_t(c)]) { reached[size_t(c)] = 1; stack.push_back(c); }
    }
    return reached;
}

int check_ids(const bn_learner* L, const char* what, int32_t count, const int32_t* ids) {
    if (count < 0 || (count > 0 && !ids)) return fail(BN_ERR_ARG, std::string("null argument or negative count: ") + what);
    for (int32_t i = 0; i < count; ++i)
        if (ids[i] < 0 || ids[i] >= L->n) return fail(BN_ERR_ARG, std::string(what) + " id " + std::to_string(ids[i]) + " out of range");
    return BN_OK;
}

// One node whose parent set an enumeration varies: its candidates (nodes that are neither the node nor a parent of it in the
// starting graph, each once), the family term of every subset of them on top of the starting parents, and the subset in hand.
struct Slot {
    int32_t node = 0, mask = 0, best_mask = 0;
    std::vector<int32_t> cand;
    std::vector<double> ll;   // [2^cand.size()], mask order
    int32_t bit_of(int32_t u) const {
        for (size_t j = 0; j < cand.size(); ++j)
            if (cand[j] == u) return int32_t(j);
        return -1;
    }
};

// The graph an enumeration walks: the learner's, plus the candidate edges in hand.  add_edge's refusals (graph.hpp:268-275: the
// edge exists or closes a cycle) and the library's limit on the number of parents.
struct Walk {
    bn_learner* L;
    std::vector<Slot> slots;
    std::vector<int32_t> slot_of;                  // per node, or -1
    std::vector<std::vector<int32_t>> children;    // the learner's, plus the edges in hand (added and removed last in, first out)
    std::vector<int32_t> n_par;
    std::vector<double> ll;                        // family term of every node in the graph in hand
    std::vector<int32_t> stamp, stack;
    int32_t now = 0;
    int64_t params = 0;

    explicit Walk(bn_learner* learner)
        : L(learner), slot_of(size_t(learner->n), -1), children(learner->children), n_par(size_t(learner->n)), ll(learner->ll),
          stamp(size_t(learner->n), 0), params(learner->params) {
        for (int32_t v = 0; v < L->n; ++v) n_par[size_t(v)] = int32_t(L->parents[size_t(v)].size());
    }

    // a slot for `node` with the nodes of `from` as candidates; one lattice call
    int add_slot(int32_t node, int32_t count, const int32_t* from) {
        if (slot_of[size_t(node)] >= 0) return BN_OK;
        Slot sl;
        sl.node = node;
        const std::vector<int32_t>& par = L->parents[size_t(node)];
        for (int32_t i = 0; i < count; ++i) {
            const int32_t u = from[i];
            if (u == node || std::binary_search(par.begin(), par.end(), u) || sl.bit_of(u) >= 0) continue;
            sl.cand.push_back(u);
        }
        if (sl.cand.size() > size_t(kLearnMaxParents))
            return fail(BN_ERR_ARG, "node " + std::to_string(node) + ": " + std::to_string(sl.cand.size()) + " candidate parents (at most " +
                                        std::to_string(kLearnMaxParents) + " minus its parents)");
        sl.ll.assign(size_t(1) << sl.cand.size(), 0.0);
        if (int r = run_subsets(L->t, L->spec, node, int32_t(par.size()), par.data(), int32_t(sl.cand.size()), sl.cand.data(), sl.ll.data(), nullptr,
                                 &L->times))
            return r;
        slot_of[size_t(node)] = int32_t(slots.size());
        slots.push_back(std::move(sl));
        return BN_OK;
    }

    bool reaches(int32_t from, int32_t to) {
        ++now;
        stack.assign(1, from);
        stamp[size_t(from)] = now;
        while (!stack.empty()) {
            const int32_t v = stack.back();
            stack.pop_back();
            if (v == to) return true;
            for (int32_t c : children[size_t(v)])
                if (stamp[size_t(c)] != now) { stamp[size_t(c)] = now; stack.push_back(c); }
        }
        return false;
    }

    // graph.add_edge(u, c): false when refused
    bool add(int32_t u, int32_t c) {
        const int32_t si = slot_of[size_t(c)];
        if (si < 0) return false;
        Slot& sl = slots[size_t(si)];
        const int32_t b = sl.bit_of(u);   // (-1: the node itself, or a parent in the starting graph)
        if (b < 0 || ((sl.mask >> b) & 1)) return false;
        if (n_par[size_t(c)] >= std::min(L->max_parents, kLearnMaxParents)) return false;
        if (reaches(c, u)) return false;
        flip(sl, b, u, c, true);
        return true;
    }
    void erase(int32_t u, int32_t c) {
        Slot& sl = slots[size_t(slot_of[size_t(c)])];
        flip(sl, sl.bit_of(u), u, c, false);
    }
    void flip(Slot& sl, int32_t b, int32_t u, int32_t c, bool on) {
        int64_t rows = 1;   // the family's rows without u
        for (int32_t x : L->parents[size_t(c)]) rows *= L->t->k[size_t(x)];
        for (size_t j = 0; j < sl.cand.size(); ++j)
            if (int32_t(j) != b && ((sl.mask >> j) & 1)) rows *= L->t->k[size_t(sl.cand[j])];
        const int64_t with = L->family_params(c, rows * L->t->k[size_t(u)]), without = L->family_params(c, rows);
        if (on) {
            sl.mask |= int32_t(1) << b;
            children[size_t(u)].push_back(c);
            ++n_par[size_t(c)];
            params += with - without;
        } else {
            sl.mask &= ~(int32_t(1) << b);
            children[size_t(u)].pop_back();
            --n_par[size_t(c)];
            params -= with - without;
        }
        ll[size_t(c)] = sl.ll[size_t(sl.mask)];
    }
    double penalised(double likelihood) const {
        if (L->criterion >= 2) return likelihood;
        return L->criterion == 0 ? likelihood + double(params) : likelihood + double(params) * L->penalty;
    }
    void keep() {
        for (Slot& sl : slots) sl.best_mask = sl.mask;
    }
    // the best graph becomes the learner's
    void commit() {
        for (const Slot& sl : slots) {
            const int32_t c = sl.node;
            std::vector<int32_t>& par = L->parents[size_t(c)];
            const int64_t before = L->family_params(c, L->rows_of(c));
            for (size_t j = 0; j < sl.cand.size(); ++j)
                if ((sl.best_mask >> j) & 1) {
                    par.insert(std::lower_bound(par.begin(), par.end(), sl.cand[j]), sl.cand[j]);
                    L->children[size_t(sl.cand[j])].push_back(c);
                }
            L->ll[size_t(c)] = sl.ll[size_t(sl.best_mask)];
            L->params += L->family_params(c, L->rows_of(c)) - before;
        }
        L->score = L->score_with(-1, 0.0, L->params);
    }
};

}  // namespace

extern "C" int bn_learn_best_parents(bn_learner* L, int32_t child, int32_t n_cand, const int32_t* cand, uint8_t* taken_out) {
    if (!L || n_cand < 0 || (n_cand > 0 && (!cand || !taken_out))) return fail(BN_ERR_ARG, "null argument or n_cand < 0");
    if (child < 0 || child >= L->n) return fail(BN_ERR_ARG, "child id " + std::to_string(child) + " out of range");
    if (int r = check_ids(L, "candidate", n_cand, cand)) return r;
    std::fill(taken_out, taken_out + n_cand, uint8_t(0));
    const std::vector<uint8_t> reached = reached_from(L, child);
    std::vector<int32_t>& par = L->parents[size_t(child)];
    const int32_t kc = L->t->k[size_t(child)];
    const int64_t rows = L->rows_of(child);
    const int32_t room = std::min(L->max_parents, kLearnMaxParents) - int32_t(par.size());
    // bn_learn_try_parents' filter: the child and what it reaches, a parent, a second listing, no room, a family over the size limit
    std::vector<int32_t> surv, surv_at;
    std::vector<uint8_t> listed(size_t(L->n), 0);
    for (int32_t i = 0; i < n_cand && room > 0; ++i) {
        const int32_t u = cand[i];
        if (reached[size_t(u)] || listed[size_t(u)] || std::binary_search(par.begin(), par.end(), u)) continue;
        if (rows * L->t->k[size_t(u)] * kc > kLearnMaxEntries) continue;
        listed[size_t(u)] = 1;
        surv.push_back(u);
        surv_at.push_back(i);
    }
    const int32_t m = int32_t(surv.size());
    if (m == 0) return BN_OK;
    if (m > kLearnMaxParents)
        return fail(BN_ERR_ARG, std::to_string(m) + " candidates may be added (at most " + std::to_string(kLearnMaxParents) + " minus the parents)");
    std::vector<double> ll(size_t(1) << m);
    if (int r = run_subsets(L->t, L->spec, child, int32_t(par.size()), par.data(), m, surv.data(), ll.data(), nullptr, &L->times)) return r;
    // the reference's visiting order (brute_force.hpp:104-111): "not added" before "added", cand[0] outermost
    int32_t best_mask = 0;
    int64_t best_params = L->params;
    double best = L->score_with(child, ll[0], L->params);
    for (int32_t r = 1; r < (int32_t(1) << m); ++r) {
        int32_t mask = 0, size = 0;
        int64_t rows_r = rows;
        for (int32_t j = 0; j < m; ++j)
            if ((r >> (m - 1 - j)) & 1) {
                mask |= int32_t(1) << j;
                ++size;
                rows_r *= L->t->k[size_t(surv[size_t(j)])];
            }
        if (size > room) continue;
        const int64_t params_r = L->params - L->family_params(child, rows) + L->family_params(child, rows_r);
        const double score_r = L->score_with(child, ll[size_t(mask)], params_r);
        if (score_r < best) {
            best = score_r;
            best_mask = mask;
            best_params = params_r;
        }
    }
    if (best_mask == 0) return BN_OK;   // the empty subset keeps the graph
    for (int32_t j = 0; j < m; ++j)
        if ((best_mask >> j) & 1) {
            par.insert(std::lower_bound(par.begin(), par.end(), surv[size_t(j)]), surv[size_t(j)]);
            L->children[size_t(surv[size_t(j)])].push_back(child);
            taken_out[surv_at[size_t(j)]] = 1;
        }
    L->ll[size_t(child)] = ll[size_t(best_mask)];
    L->params = best_params;
    L->score = best;
    return BN_OK;
}

extern "C" int bn_learn_terms(const bn_learner* L, double* ll_out, int64_t* params_out) {
    if (!L || !ll_out) return fail(BN_ERR_ARG, "null argument");
    std::copy(L->ll.begin(), L->ll.end(), ll_out);
    if (params_out) *params_out = L->params;
    return BN_OK;
}

extern "C" int bn_learn_brute_force_hint(bn_learner* L, int32_t n_par, const int32_t* par, int32_t n_child, const int32_t* child) {
    if (!L) return fail(BN_ERR_ARG, "null argument");
    if (int r = check_ids(L, "parent", n_par, par)) return r;
    if (int r = check_ids(L, "child", n_child, child)) return r;
    // no add_edge can be refused for a cycle when no child reaches a parent node (a child itself included): every new edge starts
    // at a parent node, so a path from a child to a parent node would have to exist already
    std::vector<uint8_t> is_par(size_t(L->n), 0);
    for (int32_t i = 0; i < n_par; ++i) is_par[size_t(par[i])] = 1;
    bool decomposed = true;
    for (int32_t i = 0; i < n_child && decomposed; ++i) {
        const std::vector<uint8_t> reached = reached_from(L, child[i]);
        for (int32_t v = 0; v < L->n && decomposed; ++v)
            if (reached[size_t(v)] && is_par[size_t(v)]) decomposed = false;
    }
    if (decomposed) {
        // per child the other children's edges are fixed terms of the sum, so the depth-first search is one search per child; a
        // child listed again finds its best subset in place
        std::vector<uint8_t> taken(size_t(std::max(n_par, 1)));
        std::vector<uint8_t> done(size_t(L->n), 0);
        for (int32_t i = 0; i < n_child; ++i) {
            if (done[size_t(child[i])]) continue;
            done[size_t(child[i])] = 1;
            if (int r = bn_learn_best_parents(L, child[i], n_par, par, taken.data())) return r;
        }
        return BN_OK;
    }
    const int64_t edges = int64_t(n_par) * n_child;
    if (edges > 20)
        return fail(BN_ERR_ARG, std::to_string(edges) + " possible edges with a child that reaches a parent node: the literal enumeration takes at most 20");
    Walk w(L);
    for (int32_t i = 0; i < n_child; ++i)
        if (int r = w.add_slot(child[i], n_par, par)) return r;
    double best = L->score;
    // brute_force.hpp:85-113, the possible edges parent-major (:61-67)
    struct Rec {
        Walk& w;
        const int32_t *par, *child;
        int32_t n_child;
        int64_t edges;
        double& best;
        void run(int64_t e) {
            if (e == edges) {
                double likelihood = 0.0;
                for (double x : w.ll) likelihood -= x;
                const double now = w.penalised(likelihood);
                if (now < best) {
                    best = now;
                    w.keep();
                }
                return;
            }
            run(e + 1);
            const int32_t u = par[e / n_child], c = child[e % n_child];
            if (w.add(u, c)) {
                run(e + 1);
                w.erase(u, c);
            }
        }
    } rec{w, par, child, n_child, edges, best};
    rec.run(0);
    w.commit();
    return BN_OK;
}

extern "C" int bn_learn_brute_force(bn_learner* L, int32_t n_v, const int32_t* vertexes, double* eval_out) {
    if (!L) return fail(BN_ERR_ARG, "null argument");
    if (int r = check_ids(L, "vertex", n_v, vertexes)) return r;
    if (n_v > 8) return fail(BN_ERR_ARG, std::to_string(n_v) + " vertexes (at most 8: 2 027 025 graphs)");
    for (int32_t i = 0; i < n_v; ++i)
        for (int32_t j = 0; j < i; ++j)
            if (vertexes[i] == vertexes[j]) return fail(BN_ERR_ARG, "vertex " + std::to_string(vertexes[i]) + " listed twice");
    Walk w(L);
    for (int32_t i = 0; i < n_v; ++i)
        if (int r = w.add_slot(vertexes[i], n_v, vertexes)) return r;
    // eval_(graph, vertexes): the likelihood over `vertexes` in the given order, the parameters of the whole graph
    auto eval = [&]() {
        double likelihood = 0.0;
        for (int32_t i = 0; i < n_v; ++i) likelihood -= w.ll[size_t(vertexes[i])];
        return w.penalised(likelihood);
    };
    double best = eval();
    // brute_force.hpp:116-156.  Level t tries per later vertex: no edge, v_t -> v_i, v_i -> v_t.  "No edge" gives the same graph for
    // every i, so it is walked for the first i only: a graph seen again cannot win under <.
    struct Rec {
        Walk& w;
        const int32_t* v;
        int32_t n_v;
        double& best;
        decltype(eval)& eval_;
        void run(int32_t t) {
            if (t == n_v - 1) {
                const double now = eval_();
                if (now < best) {
                    best = now;
                    w.keep();
                }
                return;
            }
            for (int32_t i = t + 1; i < n_v; ++i) {
                if (i == t + 1) run(t + 1);
                if (w.add(v[t], v[i])) {
                    run(t + 1);
                    w.erase(v[t], v[i]);
                }
                if (w.add(v[i], v[t])) {
                    run(t + 1);
                    w.erase(v[i], v[t]);
                }
            }
        }
    } rec{w, vertexes, n_v, best, eval};
    if (n_v > 0) rec.run(0);
    w.commit();
    if (eval_out) *eval_out = best;
    return BN_OK;
}

// ---- simulated annealing: the term table and the chains (reference bayesian/learning/simulated_annealing.hpp) ----------------------

struct bn_term_table {
    bn_info_table* t = nullptr;
    int device = 0;
    int32_t n = 0, q = 0;
    int64_t T = 0;                       // entries per child
    std::vector<uint32_t> tab;           // the rank tables (bn_learn_anneal.hpp)
    DeviceBuf<double> d_terms;
    DeviceBuf<uint32_t> d_tab;
    DeviceBuf<int32_t> d_k;
    int64_t ineligible = 0;
    bn_score_spec spec = kLogLikSpec;    // the family term the entries hold
    LearnTimes times;

    // sorted parents, none of them c
    int64_t rank(int32_t c, const int32_t* par, int32_t j) const {
        int64_t r = tab[size_t(j)];
        for (int32_t i = 0; i < j; ++i) r += tab[size_t(kAnnealTabBinom + (i + 1) * 64 + (par[i] - (par[i] > c ? 1 : 0)))];
        return r;
    }
    ~bn_term_table() {
        DeviceGuard g;
        (void)g.enter(device);
        d_terms.reset(); d_tab.reset(); d_k.reset();
    }
};

extern "C" int bn_terms_create(bn_info_table* t, int32_t max_parents, bn_term_table** out) {
    return bn_terms_create_spec(t, nullptr, max_parents, out);
}

extern "C" int bn_terms_create_spec(bn_info_table* t, const bn_score_spec* spec_in, int32_t max_parents, bn_term_table** out) {
    if (!out) return fail(BN_ERR_ARG, "null argument");
    *out = nullptr;
    if (!t) return fail(BN_ERR_ARG, "null argument");
    bn_score_spec spec;
    if (int r = check_spec(spec_in, spec)) return r;
    if (max_parents < 1 || max_parents > kLearnMaxParents) return fail(BN_ERR_ARG, "term table: max_parents must be in 1..16");
    const int32_t n = t->n, q = max_parents;
    if (n > kAnnealMaxNodes)
        return fail(BN_ERR_ARG, "term table: " + std::to_string(n) + " nodes (at most " + std::to_string(kAnnealMaxNodes) + ": a node has a lane)");
    // C(a, i) for a <= 63, i <= 16 (C(63, 16) < 2^49)
    std::vector<std::vector<uint64_t>> C(64, std::vector<uint64_t>(18, 0));
    for (int a = 0; a < 64; ++a) {
        C[size_t(a)][0] = 1;
        for (int i = 1; i <= 17 && i <= a; ++i) C[size_t(a)][size_t(i)] = C[size_t(a - 1)][size_t(i - 1)] + (i <= a - 1 ? C[size_t(a - 1)][size_t(i)] : 0);
    }
    std::vector<int64_t> offset(size_t(q) + 2, 0);
    for (int32_t j = 0; j <= q; ++j) {
        offset[size_t(j) + 1] = offset[size_t(j)] + int64_t(n >= 1 ? C[size_t(n - 1)][size_t(j)] : 0);
        if (offset[size_t(j) + 1] * n > kAnnealMaxEntries) {
            // (the sum only grows: name the whole table's size, in 128-bit-free arithmetic -- every term is below 2^49 and q <= 16)
            int64_t total = 0;
            for (int32_t u = 0; u <= q; ++u) total += int64_t(C[size_t(n - 1)][size_t(u)]);
            return fail(BN_ERR_ARG, "term table: " + std::to_string(n) + " nodes x " + std::to_string(total) + " parent sets of at most " +
                                        std::to_string(q) + " = " + std::to_string(total * n) + " entries (at most 2^22 = " +
                                        std::to_string(kAnnealMaxEntries) + ")");
        }
    }
    std::unique_ptr<bn_term_table> tt(new (std::nothrow) bn_term_table);
    if (!tt) return fail(BN_ERR_ALLOC, "host allocation failed");
    tt->t = t;
    tt->device = t->device;
    tt->n = n;
    tt->q = q;
    tt->spec = spec;
    tt->T = offset[size_t(q) + 1];
    tt->tab.assign(size_t(kAnnealTabWords), 0u);
    for (int32_t j = 0; j <= q; ++j) tt->tab[size_t(j)] = uint32_t(offset[size_t(j)]);
    for (int32_t i = 0; i <= q; ++i)
        for (int32_t a = 0; a + 1 < n; ++a) tt->tab[size_t(kAnnealTabBinom + i * 64 + a)] = uint32_t(C[size_t(a)][size_t(i)]);   // (<= C(n - 1, q) <= T)

    // every family once: the groups (c, B, candidates above max(B)) for every B of fewer than q nodes; a family over the per-family
    // limit is left out of the batch (its supersets too) and keeps its NaN
    std::vector<int32_t> g_child, g_base_at, g_nbase, g_cand_at, g_ncand, base_store, cand_store;
    std::vector<int32_t> B;
    for (int32_t c = 0; c < n; ++c) {
        const int64_t kc = t->k[size_t(c)];
        B.clear();
        // the subsets of the other nodes of size < q in lexicographic order, by a stack of node ids
        for (;;) {
            int64_t rows = 1;
            for (int32_t u : B) rows *= t->k[size_t(u)];
            const bool base_ok = rows * kc <= kLearnMaxEntries;
            if (base_ok) {
                const int32_t cand_at = int32_t(cand_store.size());
                for (int32_t u = B.empty() ? 0 : B.back() + 1; u < n; ++u)
                    if (u != c && rows * t->k[size_t(u)] * kc <= kLearnMaxEntries) cand_store.push_back(u);
                const int32_t n_cand = int32_t(cand_store.size()) - cand_at;
                if (B.empty() || n_cand > 0) {
                    g_child.push_back(c);
                    g_base_at.push_back(int32_t(base_store.size()));
                    g_nbase.push_back(int32_t(B.size()));
                    g_cand_at.push_back(cand_at);
                    g_ncand.push_back(n_cand);
                    base_store.insert(base_store.end(), B.begin(), B.end());
                }
            }
            // next: extend by the smallest node above the last (when the base may still grow), else advance the last, else pop
            auto next_above = [&](int32_t u) {
                ++u;
                if (u == c) ++u;
                return u;
            };
            bool moved = false;
            if (base_ok && int32_t(B.size()) + 1 < q) {
                const int32_t u = next_above(B.empty() ? -1 : B.back());
                if (u < n) {
                    B.push_back(u);
                    moved = true;
                }
            }
            while (!moved && !B.empty()) {
                const int32_t u = next_above(B.back());
                if (u < n) {
                    B.back() = u;
                    moved = true;
                } else {
                    B.pop_back();
                }
            }
            if (!moved) break;
        }
    }
    std::vector<GroupIn> groups(g_child.size());
    size_t n_fams = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
        groups[g] = GroupIn{g_child[g], base_store.data() + g_base_at[g], g_nbase[g], cand_store.data() + g_cand_at[g], g_ncand[g]};
        n_fams += size_t(1 + g_ncand[g]);
    }
    std::vector<double> ll(std::max<size_t>(n_fams, 1), 0.0);
    if (int r = run_groups(t, spec, groups, ll.data(), nullptr, &tt->times)) return r;
    std::vector<double> terms(size_t(tt->T) * size_t(n), std::numeric_limits<double>::quiet_NaN());
    {
        size_t at = 0;
        std::vector<int32_t> S;
        for (size_t g = 0; g < groups.size(); ++g) {
            const GroupIn& in = groups[g];
            if (in.n_base == 0) terms[size_t(in.child) * size_t(tt->T)] = ll[at];
            S.assign(in.base, in.base + in.n_base);
            S.push_back(0);
            for (int32_t j = 0; j < in.n_cand; ++j) {
                S.back() = in.cand[j];   // (above every base parent)
                terms[size_t(in.child) * size_t(tt->T) + size_t(tt->rank(in.child, S.data(), in.n_base + 1))] = ll[at + 1 + size_t(j)];
            }
            at += size_t(1 + in.n_cand);
        }
    }
    for (double x : terms)
        if (x != x) ++tt->ineligible;
    ON_DEVICE(t);
    int r;
    if ((r = upload(tt->d_terms, terms, t->stream)) || (r = upload(tt->d_tab, tt->tab, t->stream)) || (r = upload(tt->d_k, t->k, t->stream))) return r;
    HIPCHK(hipStreamSynchronize(t->stream));
    *out = tt.release();
    return BN_OK;
}

extern "C" void bn_terms_destroy(bn_term_table* tt) { delete tt; }

extern "C" int bn_terms_get(const bn_term_table* tt, const char* name, int64_t* out) {
    if (!tt || !name || !out) return fail(BN_ERR_ARG, "null argument");
    const std::string s(name);
    if (s == "entries") *out = tt->T * tt->n;
    else if (s == "row_entries") *out = tt->T;
    else if (s == "nodes") *out = tt->n;
    else if (s == "max_parents") *out = tt->q;
    else if (s == "ineligible") *out = tt->ineligible;
    else if (s == "families_scored") *out = tt->times.families;
    else if (s == "passes") *out = tt->times.passes;
    else if (s == "build_ns") *out = int64_t(tt->times.count_ns + tt->times.score_ns);
    else if (s == "score_kind") *out = tt->spec.kind;
    else if (s == "ess_bits") std::memcpy(out, &tt->spec.ess, 8);
    else return fail(BN_ERR_ARG, "unknown name (score_kind, ess_bits, entries, row_entries, nodes, max_parents, ineligible, families_scored, passes, build_ns)");
    return BN_OK;
}

extern "C" int bn_terms_fetch(const bn_term_table* tt, int32_t child, double* ll_out) {
    if (!tt || !ll_out) return fail(BN_ERR_ARG, "null argument");
    if (child < 0 || child >= tt->n) return fail(BN_ERR_ARG, "child id " + std::to_string(child) + " out of range");
    ON_DEVICE(tt);
    HIPCHK(hipMemcpyAsync(ll_out, tt->d_terms.get() + size_t(child) * size_t(tt->T), size_t(tt->T) * 8, hipMemcpyDeviceToHost, tt->t->stream));
    HIPCHK(hipStreamSynchronize(tt->t->stream));
    return BN_OK;
}

// the winner's graph and terms become the learner's (score = score_with(-1, 0.0, params): the kernels' evaluation is that function)
// a search over a term table reads the table's terms as the learner's: they must be the same function
static int check_table_spec(const char* who, const bn_learner* L, const bn_term_table* tt) {
    if (same_spec(L->spec, tt->spec)) return BN_OK;
    std::string what = std::string(who) + ": the term table holds " + spec_name(tt->spec) + " terms, the learner scores by " + spec_name(L->spec);
    if (L->spec.kind == 2 && tt->spec.kind == 2) what += " with another ess (" + std::to_string(tt->spec.ess) + " against " + std::to_string(L->spec.ess) + ")";
    return fail(BN_ERR_ARG, what);
}

static void adopt_winner(bn_learner* L, const std::vector<uint64_t>& win_mask, const std::vector<double>& win_ll, double score) {
    const int32_t n = L->n;
    for (int32_t v = 0; v < n; ++v) {
        L->parents[size_t(v)].clear();
        L->children[size_t(v)].clear();
    }
    L->params = 0;
    for (int32_t v = 0; v < n; ++v) {
        for (int32_t u = 0; u < n; ++u)
            if ((win_mask[size_t(v)] >> u) & 1) {
                L->parents[size_t(v)].push_back(u);
                L->children[size_t(u)].push_back(v);
            }
        L->ll[size_t(v)] = win_ll[size_t(v)];
        L->params += L->family_params(v, L->rows_of(v));
    }
    L->score = score;
}

static_assert(sizeof(bn_anneal_trace) == sizeof(AnnealTrace) && sizeof(AnnealTrace) == 16, "the trace record is the ABI's");
static_assert(sizeof(AnnealRecord) == 32, "one record per chain");

extern "C" int bn_learn_anneal(bn_learner* L, bn_term_table* tt, const bn_anneal_params* p, int32_t chains, uint64_t seed, double* eval_out,
                               uint32_t* counts_out, uint64_t* masks_out, int32_t* n_edges_out, uint16_t* edges_out,
                               bn_anneal_trace* trace_out, int32_t* winner_out) {
    if (!L || !tt || !p) return fail(BN_ERR_ARG, "null argument");
    if (tt->t != L->t) return fail(BN_ERR_ARG, "anneal: the term table was built from another table than the learner's");
    if (int r = check_table_spec("anneal", L, tt)) return r;
    auto positive = [](double x) { return std::isfinite(x) && x > 0.0; };
    if (!positive(p->initial_temp) || !positive(p->final_temp)) return fail(BN_ERR_ARG, "anneal: the temperatures must be finite and positive");
    if (!(p->decreasing_rate > 0.0 && p->decreasing_rate < 1.0)) return fail(BN_ERR_ARG, "anneal: decreasing_rate must be in (0, 1)");
    if (!positive(p->boltzmann)) return fail(BN_ERR_ARG, "anneal: boltzmann must be finite and positive");
    if (p->rule != 0 && p->rule != 1) return fail(BN_ERR_ARG, "anneal: rule 0 (the reference's) or 1 (Metropolis)");
    if (chains < 1 || chains > kAnnealMaxChains) return fail(BN_ERR_ARG, "anneal: " + std::to_string(chains) + " chains (1 .. 65536)");
    if (p->max_proposals > kAnnealMaxProposals)
        return fail(BN_ERR_ARG, "anneal: max_proposals " + std::to_string(p->max_proposals) + " (at most 2^24 = " + std::to_string(kAnnealMaxProposals) + ")");
    if (p->trace_chain < -1 || p->trace_chain >= chains) return fail(BN_ERR_ARG, "anneal: trace_chain out of range");
    const bool tracing = p->trace_chain >= 0 && trace_out && p->trace_cap > 0;
    const int32_t n = L->n, q = tt->q;
    std::vector<uint64_t> pmask(size_t(n), 0);
    std::vector<int64_t> rows(size_t(n), 1);
    std::vector<uint16_t> edges;
    for (int32_t v = 0; v < n; ++v) {
        if (int32_t(L->parents[size_t(v)].size()) > q)
            return fail(BN_ERR_ARG, "anneal: node " + std::to_string(v) + " starts with " + std::to_string(L->parents[size_t(v)].size()) +
                                        " parents (the term table holds at most " + std::to_string(q) + ")");
        for (int32_t u : L->parents[size_t(v)]) {
            pmask[size_t(v)] |= uint64_t(1) << u;
            edges.push_back(uint16_t(u | (v << 8)));
        }
        rows[size_t(v)] = L->rows_of(v);
    }
    const int32_t stride = std::max(n * q, 1);
    bn_info_table* t = L->t;
    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<uint64_t> d_pmask, d_masks;
    DeviceBuf<int64_t> d_rows;
    DeviceBuf<double> d_ll0, d_ll;
    DeviceBuf<uint16_t> d_edges0, d_edges;
    DeviceBuf<AnnealRecord> d_rec;
    DeviceBuf<AnnealTrace> d_trace;
    EventOwner ev0, ev1;
    int r;
    if ((r = upload(d_pmask, pmask, s)) || (r = upload(d_rows, rows, s)) || (r = upload(d_ll0, L->ll, s)) || (r = upload(d_edges0, edges, s)) ||
        (r = dalloc(d_rec, size_t(chains))) || (r = dalloc(d_masks, size_t(chains) * size_t(n))) || (r = dalloc(d_ll, size_t(chains) * size_t(n))))
        return r;
    if (edges_out && (r = dalloc(d_edges, size_t(chains) * size_t(stride)))) return r;
    if (tracing && (r = dalloc(d_trace, size_t(p->trace_cap)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    AnnealArgs a{};
    a.terms = tt->d_terms;
    a.tab = tt->d_tab;
    a.T = tt->T;
    a.k = tt->d_k;
    a.pmask0 = d_pmask;
    a.rows0 = d_rows;
    a.ll0 = d_ll0;
    a.edges0 = d_edges0;
    a.n_edges0 = int32_t(edges.size());
    a.n = n;
    a.q = q;
    a.max_parents = std::min(q, L->max_parents);
    a.criterion = L->criterion;
    a.rule = p->rule;
    a.params0 = L->params;
    a.penalty = L->penalty;
    a.initial_temp = p->initial_temp;
    a.final_temp = p->final_temp;
    a.rate = p->decreasing_rate;
    a.boltzmann = p->boltzmann;
    a.same_state_max = p->same_state_max;
    a.max_proposals = p->max_proposals == 0 ? (1u << 20) : p->max_proposals;
    a.seed_lo = uint32_t(seed);
    a.seed_hi = uint32_t(seed >> 32);
    a.chains = chains;
    a.trace_chain = tracing ? p->trace_chain : -1;
    a.trace_cap = tracing ? p->trace_cap : 0;
    a.rec = d_rec;
    a.masks = d_masks;
    a.ll = d_ll;
    a.edges = edges_out ? d_edges.get() : nullptr;
    a.edge_stride = stride;
    a.trace = tracing ? d_trace.get() : nullptr;
    HIPCHK(hipEventRecord(ev0, s));
    if (int err = learn_launch_anneal(a, s)) return fail(BN_ERR_HIP, std::string("annealing kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    std::vector<AnnealRecord> rec(static_cast<size_t>(chains));
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, size_t(chains) * sizeof(AnnealRecord), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int32_t winner = 0;
    int64_t steps = 0;
    for (int32_t j = 0; j < chains; ++j) {
        if (rec[size_t(j)].eval < rec[size_t(winner)].eval) winner = j;   // strictly smaller: ties stay with the lowest index
        steps += rec[size_t(j)].proposals;
    }
    std::vector<uint64_t> win_mask(static_cast<size_t>(n));
    std::vector<double> win_ll(static_cast<size_t>(n));
    HIPCHK(hipMemcpyAsync(win_mask.data(), d_masks.get() + size_t(winner) * size_t(n), size_t(n) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(win_ll.data(), d_ll.get() + size_t(winner) * size_t(n), size_t(n) * 8, hipMemcpyDeviceToHost, s));
    if (masks_out) HIPCHK(hipMemcpyAsync(masks_out, d_masks, size_t(chains) * size_t(n) * 8, hipMemcpyDeviceToHost, s));
    if (edges_out) HIPCHK(hipMemcpyAsync(edges_out, d_edges, size_t(chains) * size_t(stride) * 2, hipMemcpyDeviceToHost, s));
    if (tracing) {
        const size_t len = std::min<size_t>(rec[size_t(p->trace_chain)].operated, p->trace_cap);
        if (len > 0) HIPCHK(hipMemcpyAsync(trace_out, d_trace, len * sizeof(AnnealTrace), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    L->times.anneal_ns += double(ms) * 1e6;
    L->times.anneal_chains += chains;
    L->times.anneal_steps += steps;
    for (int32_t j = 0; j < chains; ++j) {
        const AnnealRecord& x = rec[size_t(j)];
        if (eval_out) eval_out[j] = x.eval;
        if (counts_out) {
            counts_out[4 * j] = x.proposals;
            counts_out[4 * j + 1] = x.operated;
            counts_out[4 * j + 2] = x.accepted;
            counts_out[4 * j + 3] = x.flags;
        }
        if (n_edges_out) n_edges_out[j] = int32_t(x.n_edges);
    }
    if (winner_out) *winner_out = winner;
    adopt_winner(L, win_mask, win_ll, rec[size_t(winner)].eval);
    return BN_OK;
}

// ---- hierarchical clustering with stochastic pruning (reference bayesian/learning/stepwise_structure_hc.hpp) ------------------------

static_assert(sizeof(bn_hc_trace) == sizeof(HcTrace) && sizeof(HcTrace) == 16, "the trace record is the ABI's");
static_assert(sizeof(HcRecord) == 40, "one record per run");

extern "C" int bn_learn_hc(bn_learner* L, bn_term_table* tt, const bn_hc_params* p, int32_t runs, uint64_t seed, const double* similarity,
                           double* score_out, uint32_t* counts_out, uint64_t* masks_out, bn_hc_trace* trace_out, int32_t* n_trace_out,
                           int32_t* winner_out) {
    if (!L || !tt || !p) return fail(BN_ERR_ARG, "null argument");
    if (tt->t != L->t) return fail(BN_ERR_ARG, "hc: the term table was built from another table than the learner's");
    if (int r = check_table_spec("hc", L, tt)) return r;
    const int32_t n = L->n, q = tt->q;
    if (n > kAnnealMaxNodes) return fail(BN_ERR_ARG, "hc: " + std::to_string(n) + " nodes (at most 64: a node has a lane)");
    if (runs < 1 || runs > kHcMaxRuns) return fail(BN_ERR_ARG, "hc: " + std::to_string(runs) + " runs (1 .. 65536)");
    if (!(std::isfinite(p->alpha) && p->alpha >= 0.0)) return fail(BN_ERR_ARG, "hc: alpha must be finite and >= 0");
    if (p->max_parents < 1 || p->max_parents > q)
        return fail(BN_ERR_ARG, "hc: max_parents " + std::to_string(p->max_parents) + " (1 .. " + std::to_string(q) + ", the term table's bound)");
    if (p->trace_run < -1 || p->trace_run >= runs) return fail(BN_ERR_ARG, "hc: trace_run out of range");
    const bool tracing = p->trace_run >= 0 && trace_out && p->trace_cap > 0;
    bn_info_table* t = L->t;
    std::vector<double> S(size_t(n) * size_t(n), 0.0);
    if (similarity) {
        for (int32_t x = 0; x < n; ++x)
            for (int32_t y = x + 1; y < n; ++y)
                if (std::memcmp(similarity + size_t(x) * n + y, similarity + size_t(y) * n + x, 8) != 0)
                    return fail(BN_ERR_ARG, "hc: similarity[" + std::to_string(x) + "][" + std::to_string(y) + "] and [" + std::to_string(y) +
                                                "][" + std::to_string(x) + "] differ in bits (the matrix must be symmetric)");
        std::copy(similarity, similarity + S.size(), S.begin());
    }
    int64_t params0 = 0;
    for (int32_t v = 0; v < n; ++v) params0 += L->family_params(v, 1);
    ON_DEVICE(t);
    hipStream_t s = t->stream;
    DeviceBuf<double> d_S, d_ll;
    DeviceBuf<uint64_t> d_masks;
    DeviceBuf<HcRecord> d_rec;
    DeviceBuf<HcTrace> d_trace;
    EventOwner ev0, ev1;
    int r;
    if (similarity) {
        if ((r = upload(d_S, S, s))) return r;
    } else {
        // the all-pairs mutual information stays where the kernel made it; the host sees it only for `average`
        if ((r = dalloc(d_S, S.size())) || (r = info_pair_mi_device(t, d_S, S))) return r;
    }
    // :171-186: the average of the initial similarities, one divide and one add per pair in row-major order
    double average = 0.0;
    const double pairs = double(int64_t(n) * (n - 1) / 2);
    for (int32_t x = 0; x < n; ++x)
        for (int32_t y = x + 1; y < n; ++y) average += (0.0 + S[size_t(x) * n + y] / 1.0) / pairs;
    if ((r = dalloc(d_rec, size_t(runs))) || (r = dalloc(d_masks, size_t(runs) * size_t(n))) || (r = dalloc(d_ll, size_t(runs) * size_t(n))))
        return r;
    if (tracing && (r = dalloc(d_trace, size_t(p->trace_cap)))) return r;
    HIPCHK(hipEventCreate(ev0.put()));
    HIPCHK(hipEventCreate(ev1.put()));
    HcArgs a{};
    a.terms = tt->d_terms;
    a.tab = tt->d_tab;
    a.T = tt->T;
    a.k = tt->d_k;
    a.S = d_S;
    a.n = n;
    a.q = q;
    a.max_parents = std::min(p->max_parents, L->max_parents);
    a.criterion = L->criterion;
    a.params0 = params0;
    a.penalty = L->penalty;
    a.alpha = p->alpha;
    a.average = average;
    a.seed_lo = uint32_t(seed);
    a.seed_hi = uint32_t(seed >> 32);
    a.runs = runs;
    a.trace_run = tracing ? p->trace_run : -1;
    a.trace_cap = tracing ? p->trace_cap : 0;
    a.rec = d_rec;
    a.masks = d_masks;
    a.ll = d_ll;
    a.trace = tracing ? d_trace.get() : nullptr;
    HIPCHK(hipEventRecord(ev0, s));
    if (int err = learn_launch_hc(a, s)) return fail(BN_ERR_HIP, std::string("hierarchical-clustering kernel: ") + hipGetErrorString(hipError_t(err)));
    HIPCHK(hipEventRecord(ev1, s));
    std::vector<HcRecord> rec(static_cast<size_t>(runs));
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, size_t(runs) * sizeof(HcRecord), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int32_t winner = 0;
    int64_t merges = 0;
    for (int32_t j = 0; j < runs; ++j) {
        if (rec[size_t(j)].score < rec[size_t(winner)].score) winner = j;   // strictly smaller: ties stay with the lowest run
        merges += rec[size_t(j)].merges;
    }
    std::vector<uint64_t> win_mask(static_cast<size_t>(n));
    std::vector<double> win_ll(static_cast<size_t>(n));
    HIPCHK(hipMemcpyAsync(win_mask.data(), d_masks.get() + size_t(winner) * size_t(n), size_t(n) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(win_ll.data(), d_ll.get() + size_t(winner) * size_t(n), size_t(n) * 8, hipMemcpyDeviceToHost, s));
    if (masks_out) HIPCHK(hipMemcpyAsync(masks_out, d_masks, size_t(runs) * size_t(n) * 8, hipMemcpyDeviceToHost, s));
    size_t n_trace = 0;
    if (tracing) {
        const HcRecord& x = rec[size_t(p->trace_run)];
        n_trace = std::min<size_t>(size_t(x.merges) + x.visits, p->trace_cap);
        if (n_trace > 0) HIPCHK(hipMemcpyAsync(trace_out, d_trace, n_trace * sizeof(HcTrace), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    L->times.hc_ns += double(ms) * 1e6;
    L->times.hc_runs += runs;
    L->times.hc_merges += merges;
    for (int32_t j = 0; j < runs; ++j) {
        const HcRecord& x = rec[size_t(j)];
        if (score_out) score_out[j] = x.score;
        if (counts_out) {
            uint32_t* c = counts_out + 6 * size_t(j);
            c[0] = x.merges; c[1] = x.tried; c[2] = x.kept; c[3] = x.pruned; c[4] = x.pairs_kept; c[5] = x.flags;
        }
    }
    if (n_trace_out) *n_trace_out = int32_t(n_trace);
    if (winner_out) *winner_out = winner;
    adopt_winner(L, win_mask, win_ll, rec[size_t(winner)].score);
    return BN_OK;
}
