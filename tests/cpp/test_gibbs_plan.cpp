// test_gibbs_plan.cpp -- the planner of Gibbs sampling (bayesiannetwork_amd/csrc/bn_gibbs_plan.cpp) stand-alone: compiled with that
// file alone by plain g++ (tests/test_cpp_gibbs_plan.py also builds it with -fsanitize=address,undefined), no HIP and no library.
// Every case checks the colouring (proper on the moral graph, greedy), that every node is in exactly one slot, walks the slot tables
// the way the kernel does -- every index through a bounds-checked access, every table offset inside the flat CPT array for every
// state the node and its blanket can take at random -- and compares the child strides' row_c(x) with a direct computation over the
// child's parent list.  Cases: one node, two unconnected nodes, a chain, a collider, a 3 x 3 grid, a star of 70 children, a node
// with 16 parents of mixed arities and two children, a random DAG; the limits on both sides (4096 / 4097 nodes, arities summing to
// 8192 / 8193); the launch split and the kept-sweep count for runs below, at and above the per-launch cap.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "bn_gibbs_plan.hpp"

using namespace bnmi;

static long g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static unsigned long long g_seed = 12345;
static uint32_t rnd(uint32_t below) {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t((g_seed >> 33) % below);
}

struct Model {
    std::vector<int32_t> k, in_ptr{0}, in_idx;
    std::vector<int64_t> cpt_off{0};
    int32_t n() const { return int32_t(k.size()); }
    void add(int32_t arity, std::vector<int32_t> parents) {
        int64_t rows = 1;
        for (int32_t p : parents) { in_idx.push_back(p); rows *= k.at(size_t(p)); }
        in_ptr.push_back(int32_t(in_idx.size()));
        k.push_back(arity);
        cpt_off.push_back(cpt_off.back() + rows * arity);
    }
    std::vector<int32_t> parents(int32_t v) const { return std::vector<int32_t>(in_idx.begin() + in_ptr.at(size_t(v)), in_idx.begin() + in_ptr.at(size_t(v) + 1)); }
};

static GibbsPlan plan_of(const Model& m) {
    GibbsPlan p;
    build_gibbs_plan(m.n(), m.k.data(), m.in_ptr.data(), m.in_idx.data(), m.cpt_off.data(), p);
    return p;
}

static void check_plan(const Model& m, const GibbsPlan& P) {
    const int32_t n = m.n();
    CHECK(P.ok && P.why.empty() && P.n == n && int32_t(P.colour.size()) == n && int32_t(P.slots.size()) == n);
    // the moral graph, by itself
    std::vector<std::set<int32_t>> nb{size_t(n)};
    std::vector<std::vector<int32_t>> kids{size_t(n)};
    int64_t cells = 0;
    for (int32_t v = 0; v < n; ++v) {
        std::vector<int32_t> fam = m.parents(v);
        for (int32_t p : fam) kids.at(size_t(p)).push_back(v);
        fam.push_back(v);
        for (int32_t a : fam)
            for (int32_t b : fam)
                if (a != b) nb.at(size_t(a)).insert(b);
        cells += m.k[size_t(v)];
    }
    CHECK(P.cells == cells);
    // proper and greedy
    for (int32_t v = 0; v < n; ++v) {
        const int32_t c = P.colour.at(size_t(v));
        CHECK(c >= 0 && c < P.n_colours);
        std::set<int32_t> lower;   // the colours of the neighbours that were coloured before v
        for (int32_t u : nb[size_t(v)]) {
            CHECK(P.colour.at(size_t(u)) != c);
            if (u < v) lower.insert(P.colour[size_t(u)]);
        }
        CHECK(lower.count(c) == 0);
        for (int32_t q = 0; q < c; ++q) CHECK(lower.count(q) == 1);
    }
    // colour c owns slots [colour_ptr[c], colour_ptr[c + 1]) in ascending node index; every node in exactly one slot
    CHECK(int32_t(P.colour_ptr.size()) == P.n_colours + 1 && P.colour_ptr.front() == 0 && P.colour_ptr.back() == n);
    std::vector<int32_t> seen(size_t(n), 0);
    int32_t largest = 0;
    for (int32_t c = 0; c < P.n_colours; ++c) {
        CHECK(P.colour_ptr.at(size_t(c)) < P.colour_ptr.at(size_t(c) + 1));
        largest = std::max(largest, P.colour_ptr[size_t(c) + 1] - P.colour_ptr[size_t(c)]);
        for (int32_t q = P.colour_ptr[size_t(c)]; q < P.colour_ptr[size_t(c) + 1]; ++q) {
            const GibbsSlot& s = P.slots.at(size_t(q));
            CHECK(s.node >= 0 && s.node < n && P.colour[size_t(s.node)] == c);
            CHECK(q == P.colour_ptr[size_t(c)] || P.slots[size_t(q) - 1].node < s.node);
            ++seen.at(size_t(s.node));
        }
    }
    CHECK(largest == P.max_class);
    for (int32_t v = 0; v < n; ++v) CHECK(seen[size_t(v)] == 1);
    // the walk of the kernel, on three random assignments
    int64_t hist_off = 0;
    std::vector<int64_t> noff(size_t(n), 0);
    for (int32_t v = 0; v < n; ++v) { noff[size_t(v)] = hist_off; hist_off += m.k[size_t(v)]; }
    int64_t reads = 0;
    for (int rep = 0; rep < 3; ++rep) {
        std::vector<int32_t> st(static_cast<size_t>(n));
        for (int32_t v = 0; v < n; ++v) st[size_t(v)] = int32_t(rnd(uint32_t(m.k[size_t(v)])));
        for (const GibbsSlot& s : P.slots) {
            const int32_t v = s.node;
            CHECK(s.k == m.k[size_t(v)] && s.cpt_off == m.cpt_off[size_t(v)] && s.hist_off == noff[size_t(v)]);
            CHECK(s.hist_off + s.k <= P.cells);
            // the node's own row against the parent list, first parent most significant
            const std::vector<int32_t> ps = m.parents(v);
            CHECK(s.term_n == int32_t(ps.size()));
            int64_t row = 0, direct = 0;
            for (int32_t j = 0; j < s.term_n; ++j) {
                const GibbsTerm& t = P.terms.at(size_t(s.term_lo + j));
                CHECK(t.node == ps[size_t(j)]);
                row += int64_t(st.at(size_t(t.node))) * t.stride;
            }
            for (int32_t p : ps) direct = direct * m.k[size_t(p)] + st[size_t(p)];
            CHECK(row == direct);
            CHECK(s.cpt_off + row * s.k + s.k <= m.cpt_off[size_t(v) + 1]);
            // the children, ascending, and row_c(x) for every x
            CHECK(s.child_n == int32_t(kids[size_t(v)].size()));
            for (int32_t j = 0; j < s.child_n; ++j) {
                const GibbsChild& c = P.children.at(size_t(s.child_lo + j));
                CHECK(c.node == kids[size_t(v)][size_t(j)] && c.k == m.k[size_t(c.node)] && c.cpt_off == m.cpt_off[size_t(c.node)]);
                const std::vector<int32_t> cps = m.parents(c.node);
                CHECK(c.term_n == int32_t(cps.size()) - 1 && c.stride >= 1);
                int64_t base = 0;
                std::vector<int32_t> others;
                for (int32_t q = 0; q < c.term_n; ++q) {
                    const GibbsTerm& t = P.terms.at(size_t(c.term_lo + q));
                    CHECK(t.node != v);
                    others.push_back(t.node);
                    base += int64_t(st.at(size_t(t.node))) * t.stride;
                }
                std::vector<int32_t> expect_others;
                for (int32_t p : cps)
                    if (p != v) expect_others.push_back(p);
                CHECK(others == expect_others);
                for (int32_t x = 0; x < s.k; ++x) {
                    int64_t want = 0;
                    for (int32_t p : cps) want = want * m.k[size_t(p)] + (p == v ? x : st[size_t(p)]);
                    const int64_t got = base + int64_t(x) * c.stride;
                    CHECK(got == want);
                    CHECK(c.cpt_off + got * c.k + st[size_t(c.node)] < m.cpt_off[size_t(c.node) + 1]);
                }
            }
            if (rep == 0) reads += int64_t(s.k) * (1 + s.child_n);
        }
    }
    CHECK(reads == P.reads_per_sweep);
    // the launch shape
    // a chain: the power of two of lanes, 8 .. 64, that covers the largest colour class -- wider only where the states of
    // 256 / lanes chains would outgrow the LDS budget; one step narrower breaks one of the two
    const int32_t L = P.lanes_per_chain;
    CHECK(P.threads == 256 && (L == 8 || L == 16 || L == 32 || L == 64) && P.chains_per_block * L == P.threads);
    CHECK(L == 64 || L >= P.max_class);
    CHECK(L == 8 || L / 2 < P.max_class || ((4 * P.cells + 15) & ~15) + (2 * P.chains_per_block) * P.state_stride > kGibbsLdsBudget);
    CHECK(P.lds_bytes <= kGibbsLdsBudget);
    CHECK(P.state_stride >= n && P.state_stride % 16 == 0);
    CHECK(P.lds_bytes >= 4 * P.cells + P.chains_per_block * P.state_stride && P.lds_bytes % 16 == 0 && P.lds_bytes <= 64 * 1024);
    CHECK(P.default_sweeps >= 1 && P.default_sweeps <= kGibbsDefaultSweeps);
}

static void check_split(uint64_t begin, uint64_t n_sweeps, int64_t cap, uint64_t burn_in, uint64_t thin) {
    const std::vector<GibbsLaunch> L = gibbs_launches(begin, n_sweeps, cap);
    uint64_t at = begin, kept = 0;
    for (const GibbsLaunch& l : L) {
        CHECK(l.begin == at && l.count >= 1 && l.count <= uint64_t(std::max<int64_t>(cap, 1)));
        at += l.count;
        kept += gibbs_kept_sweeps(l.begin, l.count, burn_in, thin);   // the launches' kept sweeps add up to the run's
    }
    CHECK(at == begin + n_sweeps);
    CHECK(L.size() == (n_sweeps + uint64_t(std::max<int64_t>(cap, 1)) - 1) / uint64_t(std::max<int64_t>(cap, 1)));
    uint64_t direct = 0;
    for (uint64_t g = begin; g < begin + n_sweeps; ++g) direct += (g >= burn_in && (g - burn_in) % thin == 0);
    CHECK(kept == direct && gibbs_kept_sweeps(begin, n_sweeps, burn_in, thin) == direct);
}

int main() {
    int cases = 0;
    {   // one node; two unconnected nodes: one colour
        Model m; m.add(3, {});
        GibbsPlan P = plan_of(m); check_plan(m, P); CHECK(P.n_colours == 1); ++cases;
        m.add(2, {});
        P = plan_of(m); check_plan(m, P); CHECK(P.n_colours == 1 && P.max_class == 2 && P.lanes_per_chain == 8 && P.chains_per_block == 32); ++cases;
    }
    {   // a chain of five: two colours, alternating
        Model m; m.add(2, {}); for (int32_t v = 1; v < 5; ++v) m.add(2 + v % 3, {v - 1});
        const GibbsPlan P = plan_of(m); check_plan(m, P);
        CHECK(P.n_colours == 2 && P.colour == (std::vector<int32_t>{0, 1, 0, 1, 0})); ++cases;
    }
    {   // a collider: the parents are married, three colours
        Model m; m.add(2, {}); m.add(3, {}); m.add(4, {0, 1});
        const GibbsPlan P = plan_of(m); check_plan(m, P);
        CHECK(P.n_colours == 3); ++cases;
    }
    {   // a 3 x 3 grid, node (r, c) <- (r - 1, c), (r, c - 1)
        Model m;
        for (int32_t r = 0; r < 3; ++r)
            for (int32_t c = 0; c < 3; ++c) {
                std::vector<int32_t> ps;
                if (r > 0) ps.push_back((r - 1) * 3 + c);
                if (c > 0) ps.push_back(r * 3 + c - 1);
                m.add(3, ps);
            }
        const GibbsPlan P = plan_of(m); check_plan(m, P); ++cases;
    }
    {   // a star: 70 children of one colour, more than a wave has lanes
        Model m; m.add(3, {}); for (int32_t c = 0; c < 70; ++c) m.add(2, {0});
        const GibbsPlan P = plan_of(m); check_plan(m, P);
        CHECK(P.n_colours == 2 && P.max_class == 70 && P.slots.at(0).child_n == 70 && P.lanes_per_chain == 64); ++cases;
    }
    {   // 16 parents of mixed arities (2^8 x 3^8 rows), a second child that shares some of them
        Model m;
        for (int32_t p = 0; p < 16; ++p) m.add(2 + p % 2, {});
        std::vector<int32_t> all(16); for (int32_t p = 0; p < 16; ++p) all[size_t(p)] = p;
        m.add(5, all);
        m.add(7, {3, 8, 15, 16});
        const GibbsPlan P = plan_of(m); check_plan(m, P);
        CHECK(P.n_colours == 17 && P.colour.at(16) == 16 && P.colour.at(17) == 0); ++cases;   // (the 16 married parents, their child)
    }
    {   // a random DAG of 300 nodes, up to four parents from the 12 nodes before
        Model m;
        for (int32_t v = 0; v < 300; ++v) {
            std::set<int32_t> ps;
            const uint32_t want = rnd(5);
            for (uint32_t q = 0; q < want && v > 0; ++q) ps.insert(v - 1 - int32_t(rnd(uint32_t(std::min(v, 12)))));
            m.add(2 + int32_t(rnd(4)), std::vector<int32_t>(ps.begin(), ps.end()));
        }
        const GibbsPlan P = plan_of(m); check_plan(m, P); ++cases;
    }
    {   // the limits: 4096 one-state nodes are taken, 4097 refused with a reason; arities summing to 8192 / 8193 the same
        Model m; for (int32_t v = 0; v < 4096; ++v) m.add(1, {});
        GibbsPlan P = plan_of(m); check_plan(m, P); CHECK(P.lanes_per_chain == 64 && P.lds_bytes == 4 * 4096 + 4 * 4096);
        m.add(1, {});
        P = plan_of(m);
        CHECK(!P.ok && P.why.find("4097 nodes") != std::string::npos && P.slots.empty()); ++cases;
        Model w; for (int32_t v = 0; v < 4096; ++v) w.add(2, v % 2 ? std::vector<int32_t>{v - 1} : std::vector<int32_t>{});
        P = plan_of(w); check_plan(w, P); CHECK(P.cells == 8192 && P.lanes_per_chain == 64 && P.lds_bytes == 4 * 8192 + 4 * 4096 && P.lds_bytes <= 48 * 1024);   // (2 048 nodes a colour)
        Model x; for (int32_t v = 0; v < 4095; ++v) x.add(2, {});
        x.add(3, {});
        P = plan_of(x);
        CHECK(!P.ok && P.why.find("8193") != std::string::npos && P.slots.empty()); ++cases;
    }
    // the launch split: below, at and above the cap, a cap of one, none, no sweeps at all; burn-in inside, before and beyond
    for (uint64_t begin : {uint64_t(0), uint64_t(5), (uint64_t(1) << 32) - 40})
        for (uint64_t n_sweeps : {uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(4), uint64_t(10), uint64_t(31)})
            for (int64_t cap : {int64_t(0), int64_t(1), int64_t(3), int64_t(10), int64_t(256)})
                for (uint64_t burn_in : {uint64_t(0), begin + 2, begin + 100})
                    for (uint64_t thin : {uint64_t(1), uint64_t(3), uint64_t(7)}) check_split(begin, n_sweeps, cap, burn_in, thin);
    CHECK(gibbs_blocks(0, 4) == 0 && gibbs_blocks(1, 4) == 1 && gibbs_blocks(4, 4) == 1 && gibbs_blocks(5, 4) == 2 && gibbs_blocks(67, 4) == 17 &&
          gibbs_blocks(67, 32) == 3 && gibbs_blocks(64, 32) == 2);
    std::printf("ok: %d cases, %ld checks\n", cases, g_checks);
    return 0;
}
