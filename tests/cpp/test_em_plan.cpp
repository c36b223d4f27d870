// test_em_plan.cpp -- how the pattern rows of an EM E-step are cut into launches and where the 256-blocks of the E sum close
// (bn_policy::em_plan / em_chunk, bayesiannetwork_amd/csrc/bn_engine_policy.cpp), stand-alone: compiled together with
// bn_engine_policy.cpp by plain g++ (tests/test_cpp_em_plan.py also builds it with -fsanitize=address,undefined), no HIP and no
// library.  The expected values come from the rule as the header states it -- rows per launch = scratch cells / entries, at least 1,
// at most 65 536 and the table; a block closes at its 256th row and the last one at the table's last row -- worked out by hand, and
// from replaying the accumulating kernel's bookkeeping (one sum in hand, carried across launches) against one pass over the whole
// table.  Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
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

// the accumulating kernel's rule for one entry, chunk by chunk, with weights that make every order of additions visible: the list
// of (block sums) it produces must be the one a single pass over the table gives
static std::vector<std::vector<int64_t>> blocks_by_chunks(int64_t n_patterns, int32_t entries, int64_t scratch) {
    const EmPlan p = em_plan(n_patterns, entries, scratch);
    std::vector<std::vector<int64_t>> closed;
    std::vector<int64_t> hand;
    int64_t rows = 0, closes = 0;
    for (int64_t c = 0; c < p.n_chunks; ++c) {
        const EmChunk k = em_chunk(p, n_patterns, c);
        CHECK(k.first == rows && k.count >= 1 && k.count <= p.chunk);
        CHECK(k.opens_inside == !hand.empty());
        CHECK(int64_t(k.count) * entries <= p.scratch);
        int32_t closed_here = 0;
        for (int64_t g = k.first; g < k.first + k.count; ++g) {
            hand.push_back(g);
            if (g % kEmBlock == kEmBlock - 1 || g == n_patterns - 1) { closed.push_back(hand); hand.clear(); ++closed_here; }
        }
        CHECK(closed_here == k.closes);
        rows += k.count;
        closes += k.closes;
    }
    CHECK(rows == n_patterns && hand.empty() && closes == p.n_blocks);
    return closed;
}

int main() {
    // ---- rows per launch: scratch / entries, at least one, at most the table and 65 536
    CHECK(em_plan(1000, 100, 300).chunk == 3);
    CHECK(em_plan(1000, 100, 300).n_chunks == 334);
    CHECK(em_plan(1000, 100, 300).scratch == 300);
    CHECK(em_plan(1000, 100, 299).chunk == 2);
    CHECK(em_plan(1000, 100, 99).chunk == 1);          // less than one row fits: still one row per launch
    CHECK(em_plan(1000, 100, 0).chunk == 1);
    CHECK(em_plan(5, 100, 1 << 20).chunk == 5);        // the table is smaller than the scratch array
    CHECK(em_plan(5, 100, 1 << 20).n_chunks == 1);
    CHECK(em_plan(1 << 20, 1, int64_t(1) << 40).chunk == kEmMaxChunk);
    CHECK(em_plan(1 << 20, 1, int64_t(1) << 40).n_chunks == 16);
    CHECK(em_plan(4096, 752, kEmScratchCells).n_chunks == 1);   // 4 096 rows of an ALARM-sized network: one launch by default
    // ---- blocks of the E sum
    CHECK(em_plan(1, 7, 100).n_blocks == 1);
    CHECK(em_plan(255, 7, 100).n_blocks == 1);
    CHECK(em_plan(256, 7, 100).n_blocks == 1);
    CHECK(em_plan(257, 7, 100).n_blocks == 2);
    CHECK(em_plan(513, 7, 100).n_blocks == 3);
    // ---- a chunk by hand: 513 rows, 100 rows per launch -> chunks at 0, 100, ..., 500; blocks close at rows 255, 511 and 512
    {
        const EmPlan p = em_plan(513, 3, 300);
        CHECK(p.chunk == 100 && p.n_chunks == 6);
        CHECK(em_chunk(p, 513, 0).closes == 0 && !em_chunk(p, 513, 0).opens_inside);
        CHECK(em_chunk(p, 513, 2).first == 200 && em_chunk(p, 513, 2).count == 100 && em_chunk(p, 513, 2).closes == 1 && em_chunk(p, 513, 2).opens_inside);
        CHECK(em_chunk(p, 513, 4).closes == 0);
        CHECK(em_chunk(p, 513, 5).first == 500 && em_chunk(p, 513, 5).count == 13 && em_chunk(p, 513, 5).closes == 2);
    }
    {
        const EmPlan p = em_plan(512, 3, 3 * 256);   // chunk edges ON the block edges
        CHECK(p.chunk == 256 && p.n_chunks == 2);
        CHECK(em_chunk(p, 512, 0).closes == 1 && em_chunk(p, 512, 1).closes == 1 && !em_chunk(p, 512, 1).opens_inside);
    }
    // ---- the result does not depend on the cut: every chunking closes the same blocks with the same rows in the same order
    const int64_t sizes[] = {1, 2, 255, 256, 257, 511, 512, 513, 1000, 1025};
    const int64_t scratches[] = {0, 3, 7 * 3, 100 * 3, 255 * 3, 256 * 3, 257 * 3, 1 << 20};
    for (int64_t n : sizes) {
        const std::vector<std::vector<int64_t>> whole = blocks_by_chunks(n, 3, int64_t(1) << 30);
        CHECK(int64_t(whole.size()) == (n + 255) / 256);
        for (size_t b = 0; b < whole.size(); ++b) {
            CHECK(whole[b].front() == int64_t(b) * 256);
            CHECK(whole[b].back() == (b + 1 == whole.size() ? n - 1 : int64_t(b) * 256 + 255));
        }
        for (int64_t sc : scratches) CHECK(blocks_by_chunks(n, 3, sc) == whole);
    }
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
