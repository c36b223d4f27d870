// bn_learn_terms.cpp -- bn_term_table (include/bn_mi355x.h, bn_terms_*): the family term of EVERY parent set of at most q nodes per
// child, made by one batch of run_groups (bn_learn_batch.cpp) and kept on the device for the searches of bn_learn_search.cpp.
#include "bn_learn_internal.hpp"
#include "bn_learn_terms.hpp"

// sorted parents, none of them c
int64_t bn_term_table::rank(int32_t c, const int32_t* par, int32_t j) const {
    int64_t r = tab[size_t(j)];
    for (int32_t i = 0; i < j; ++i) r += tab[size_t(kTermTabBinom + (i + 1) * 64 + (par[i] - (par[i] > c ? 1 : 0)))];
    return r;
}

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
    if (n > kTermMaxNodes)
        return fail(BN_ERR_ARG, "term table: " + std::to_string(n) + " nodes (at most " + std::to_string(kTermMaxNodes) + ": a node has a lane)");
    // C(a, i) for a <= 63, i <= 16 (C(63, 16) < 2^49)
    std::vector<std::vector<uint64_t>> C(64, std::vector<uint64_t>(18, 0));
    for (int a = 0; a < 64; ++a) {
        C[size_t(a)][0] = 1;
        for (int i = 1; i <= 17 && i <= a; ++i) C[size_t(a)][size_t(i)] = C[size_t(a - 1)][size_t(i - 1)] + (i <= a - 1 ? C[size_t(a - 1)][size_t(i)] : 0);
    }
    std::vector<int64_t> offset(size_t(q) + 2, 0);
    for (int32_t j = 0; j <= q; ++j) {
        offset[size_t(j) + 1] = offset[size_t(j)] + int64_t(n >= 1 ? C[size_t(n - 1)][size_t(j)] : 0);
        if (offset[size_t(j) + 1] * n > kTermMaxEntries) {
            // (the sum only grows: name the whole table's size, in 128-bit-free arithmetic -- every term is below 2^49 and q <= 16)
            int64_t total = 0;
            for (int32_t u = 0; u <= q; ++u) total += int64_t(C[size_t(n - 1)][size_t(u)]);
            return fail(BN_ERR_ARG, "term table: " + std::to_string(n) + " nodes x " + std::to_string(total) + " parent sets of at most " +
                                        std::to_string(q) + " = " + std::to_string(total * n) + " entries (at most 2^22 = " +
                                        std::to_string(kTermMaxEntries) + ")");
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
    tt->tab.assign(size_t(kTermTabWords), 0u);
    for (int32_t j = 0; j <= q; ++j) tt->tab[size_t(j)] = uint32_t(offset[size_t(j)]);
    for (int32_t i = 0; i <= q; ++i)
        for (int32_t a = 0; a + 1 < n; ++a) tt->tab[size_t(kTermTabBinom + i * 64 + a)] = uint32_t(C[size_t(a)][size_t(i)]);   // (<= C(n - 1, q) <= T)

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
