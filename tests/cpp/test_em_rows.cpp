// test_em_rows.cpp -- the M-step's row array (bn_policy::em_rows, bayesiannetwork_amd/csrc/bn_engine_policy.cpp): for every entry of
// the flat CPT array, the first entry of the CPT row it is normalised in and the node's arity.  Stand-alone: compiled together with
// bn_engine_policy.cpp by plain g++ (tests/test_cpp_em_rows.py also builds it with -fsanitize=address,undefined), no HIP and no
// library.  The expected values come from the layout of the flat array -- a node's table is its parent assignments in order, each a
// row of k[v] consecutive entries -- worked out by hand, and from the three properties every entry must have.  Exit status 0 and
// "ok: ..." on success, the first violated expectation otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bn_engine_policy.hpp"

using namespace bn_policy;

static long g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// the array of a network, with the three properties checked on every entry
static std::vector<EmRow> rows_of(const std::vector<int64_t>& cpt_off, const std::vector<int32_t>& k) {
    const int32_t n = int32_t(k.size());
    const std::vector<EmRow> rows = em_rows(n, cpt_off.data(), k.data());
    CHECK(int64_t(rows.size()) == cpt_off[size_t(n)]);
    for (int32_t v = 0; v < n; ++v)
        for (int64_t q = cpt_off[size_t(v)]; q < cpt_off[size_t(v) + 1]; ++q) {
            const EmRow r = rows[size_t(q)];
            CHECK(r.first <= q && q < int64_t(r.first) + r.k);
            CHECK((q - cpt_off[size_t(v)]) % r.k == q - r.first);
            CHECK(r.k == k[size_t(v)]);
        }
    return rows;
}

int main() {
    {   // a lone root of arity 1: one entry, a row of its own
        const std::vector<EmRow> r = rows_of({0, 1}, {1});
        CHECK(r.size() == 1 && r[0].first == 0 && r[0].k == 1);
    }
    {   // a root of arity 2
        const std::vector<EmRow> r = rows_of({0, 2}, {2});
        CHECK(r[0].first == 0 && r[1].first == 0 && r[0].k == 2 && r[1].k == 2);
    }
    {   // parents of arities 2 and 3 (two roots in front), own arity 4: 24 entries from 5 on, `first` steps by 4
        const std::vector<EmRow> r = rows_of({0, 2, 5, 29}, {2, 3, 4});
        for (int q = 5; q < 29; ++q) {
            CHECK(r[size_t(q)].k == 4);
            CHECK(r[size_t(q)].first == 5 + (q - 5) / 4 * 4);
        }
        CHECK(r[5].first == 5 && r[8].first == 5 && r[9].first == 9 && r[28].first == 25);
        CHECK(r[2].first == 2 && r[4].first == 2 && r[4].k == 3);
    }
    {   // mixed arities back to back: a root of arity 3, then a child of it with arity 2 (first entry 3: no multiple of 3 ... or of 2),
        // then a child of that one with arity 5 (first entry 9)
        const std::vector<EmRow> r = rows_of({0, 3, 9, 19}, {3, 2, 5});
        CHECK(r[3].first == 3 && r[4].first == 3 && r[5].first == 5 && r[8].first == 7 && r[8].k == 2);
        CHECK(r[9].first == 9 && r[13].first == 9 && r[14].first == 14 && r[18].first == 14 && r[18].k == 5);
    }
    {   // entries beyond 65 535 (what a 16-bit `first` could not hold): a synthetic offset table, node 1 of arity 3 starting at 65 534
        const std::vector<EmRow> r = rows_of({0, 65534, 65534 + 300, 65534 + 300 + 70000}, {2, 3, 7});
        CHECK(r[65533].first == 65532 && r[65533].k == 2);
        CHECK(r[65534].first == 65534 && r[65536].first == 65534 && r[65537].first == 65537 && r[65537].k == 3);
        CHECK(r[65834].first == 65834 && r[65834 + 69999].first == 65834 + 69993 && r[65834 + 69999].k == 7);
    }
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
