// bn_learn.cpp -- C ABI of structure learning (include/bn_mi355x.h, bn_learn_*), reference bayesian/learning/greedy.hpp and
// k2_algorithm.hpp.  Kernels: bn_learn_kernels.hip.  bn_learn_score_groups scores batches of candidate families of a child against a
// device-resident pattern table; bn_learner holds a graph, every node's family term and the score, and bn_learn_try_parents is the
// reference's inner loop for one child with one device pass per ACCEPTED edge (plus one) instead of one fit and one score of the whole
// graph per candidate.  The logarithm is the device's fp64 log: the learner's score is its own stated function of the counts.
#include <cmath>
#include <memory>

#include "bn_engine_internal.hpp"
#include "bn_info_table.hpp"
#include "bn_learn.hpp"
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
};

std::string gname(size_t g) { return "group " + std::to_string(g) + ": "; }

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
int run_groups(bn_info_table* t, const std::vector<GroupIn>& groups, double* ll_out, uint64_t* counts_out, LearnTimes* times) {
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
        if (int err = learn_launch_score(a, int32_t(fam_at), int32_t(fam_end - fam_at), s))
            return fail(BN_ERR_HIP, std::string("family score kernel: ") + hipGetErrorString(hipError_t(err)));
        HIPCHK(hipEventRecord(ev2, s));
        HIPCHK(hipStreamSynchronize(s));
        if (times) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
            times->count_ns += double(ms) * 1e6;
            HIPCHK(hipEventElapsedTime(&ms, ev1, ev2));
            times->score_ns += double(ms) * 1e6;
        }
        fam_at = fam_end;
    }
    std::vector<double> ll(n_fams);
    HIPCHK(hipMemcpyAsync(ll.data(), d_ll, n_fams * 8, hipMemcpyDeviceToHost, s));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, d_out, size_t(out_cells) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n_fams; ++i) ll_out[size_t(order[i])] = ll[i];
    if (times) {
        times->families += int64_t(n_fams);
        times->passes += 1;
        for (const LearnChunk& c : chunks) times->count_bytes += t->P * int64_t(8 + c.n_base + 1 + c.n_cand);
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
    double penalty = 1.0;    // per parameter: 1 (AIC), log2(total) / 2 (MDL)
    double score = 0.0;
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
        return criterion == 0 ? likelihood + double(params_now) : likelihood + double(params_now) * penalty;
    }
};

extern "C" int bn_learn_score_groups(bn_info_table* t, int32_t n_groups, const int32_t* child, const int32_t* base_ptr,
                                     const int32_t* base_idx, const int32_t* cand_ptr, const int32_t* cand_idx, double* ll_out,
                                     uint64_t* counts_out) {
    if (!t || !ll_out) return fail(BN_ERR_ARG, "null argument");
    if (n_groups < 0) return fail(BN_ERR_ARG, "n_groups < 0");
    if (n_groups > 0 && (!child || !base_ptr || !cand_ptr)) return fail(BN_ERR_ARG, "null argument");
    std::vector<GroupIn> groups(static_cast<size_t>(n_groups));
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t b0 = base_ptr[g], b1 = base_ptr[g + 1], c0 = cand_ptr[g], c1 = cand_ptr[g + 1];
        if (b0 < 0 || b1 < b0 || c0 < 0 || c1 < c0 || (b1 > b0 && !base_idx) || (c1 > c0 && !cand_idx))
            return fail(BN_ERR_ARG, gname(size_t(g)) + "bad parent or candidate list");
        groups[size_t(g)] = GroupIn{child[g], base_idx ? base_idx + b0 : nullptr, b1 - b0, cand_idx ? cand_idx + c0 : nullptr, c1 - c0};
    }
    return run_groups(t, groups, ll_out, counts_out, nullptr);
}

extern "C" int bn_learn_create(bn_info_table* t, const int32_t* in_ptr, const int32_t* in_idx, int32_t criterion, int32_t max_parents,
                               bn_learner** out) {
    if (!out) return fail(BN_ERR_ARG, "null argument");
    *out = nullptr;
    if (!t || !in_ptr) return fail(BN_ERR_ARG, "null argument");
    if (criterion != 0 && criterion != 1) return fail(BN_ERR_ARG, "criterion: 0 AIC, 1 MDL");
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
    L->max_parents = max_parents;
    L->penalty = criterion == 0 ? 1.0 : std::log2(t->Nd) / 2;
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
    if (int r = run_groups(t, groups, L->ll.data(), nullptr, &L->times)) return r;   // (names the node as "group v" when over a limit)
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
        if (int r = run_groups(L->t, group, ll.data(), nullptr, &L->times)) return r;
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
    else if (s == "edges") {
        *out = 0;
        for (const auto& p : L->parents) *out += int64_t(p.size());
    } else if (s == "parameters") *out = L->params;
    else return fail(BN_ERR_ARG, "unknown name (families_scored, passes, count_ns, score_ns, count_bytes, edges, parameters)");
    return BN_OK;
}
