// test_memo0_policy.cpp -- the host decisions of the resident path's first-sweep image (bn_policy::memo0_*, bayesiannetwork_amd/csrc/
// bn_engine_policy.cpp), stand-alone: compiled together with bn_engine_policy.cpp by plain g++ (tests/test_cpp_memo0_policy.py builds
// it with -fsanitize=address,undefined), no HIP and no library.  Three questions: does a run start from the image; which nodes of the
// image go back to "no evidence" when a new set replaces the one applied before; what is the part of sweep 0's residual that the
// nodes without evidence contribute.  The expected values are written out from the rules -- the image is used only when it is
// valid, the option is on, the launch is the grid-barrier form, max_sweeps is 0 or >= 2 and eps <= a finite positive constant part
// (the stop test is residual < eps); the restore list is the old set minus the new one in the old set's order; the constant part is
// the contribution of the first node, by descending contribution, that the new set does not list -- not from running the functions.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

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

static Memo0Run run(bool enabled, bool valid, bool flow, int32_t max_sweeps, double eps, double c) {
    Memo0Run r;
    r.enabled = enabled; r.image_valid = valid; r.flow = flow; r.max_sweeps = max_sweeps; r.eps = eps; r.const_residual = c;
    return r;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- whether a run uses the image
    CHECK(memo0_applies(run(true, true, false, 0, 1e-3, 0.75)));
    CHECK(!memo0_applies(run(false, true, false, 0, 1e-3, 0.75)));    // option off
    CHECK(!memo0_applies(run(true, false, false, 0, 1e-3, 0.75)));    // no image
    CHECK(!memo0_applies(run(true, true, true, 0, 1e-3, 0.75)));      // dataflow form / shard
    CHECK(!memo0_applies(run(true, true, false, 1, 1e-3, 0.75)));     // the run ends behind sweep 0
    CHECK(memo0_applies(run(true, true, false, 2, 1e-3, 0.75)));
    CHECK(memo0_applies(run(true, true, false, 1030, 0.0, 0.75)));
    CHECK(memo0_applies(run(true, true, false, 0, 0.75, 0.75)));      // residual < eps stops: eps == the constant part does not
    CHECK(!memo0_applies(run(true, true, false, 0, std::nextafter(0.75, 1.0), 0.75)));
    CHECK(!memo0_applies(run(true, true, false, 0, 0.9, 0.75)));
    CHECK(!memo0_applies(run(true, true, false, 0, 1e-3, 0.0)));      // every node carries evidence
    CHECK(!memo0_applies(run(true, true, false, 0, 1e-3, -1.0)));
    CHECK(!memo0_applies(run(true, true, false, 0, 1e-3, inf)));
    CHECK(!memo0_applies(run(true, true, false, 0, 1e-3, nan)));
    CHECK(!memo0_applies(run(true, true, false, 0, nan, 0.75)));
    CHECK(memo0_applies(run(true, true, false, 0, -1.0, 0.75)));      // (eps <= 0 never stops a run)

    // ---- membership stamps and the restore list
    std::vector<uint32_t> stamp;
    uint32_t epoch = 0;
    std::vector<int32_t> out, applied;
    const int32_t n = 10;
    const int32_t A[] = {1, 4, 7, 9};
    memo0_stamp(A, 4, n, stamp, epoch);
    CHECK(stamp.size() == 10 && epoch == 1 && stamp[4] == 1 && stamp[0] == 0);
    memo0_restore_list(applied, stamp, epoch, out);                   // nothing applied before
    CHECK(out.empty());
    applied.assign(A, A + 4);
    const int32_t B[] = {9, 2, 4};                                    // shares 4 and 9, drops 1 and 7, adds 2
    memo0_stamp(B, 3, n, stamp, epoch);
    CHECK(epoch == 2);
    memo0_restore_list(applied, stamp, epoch, out);
    CHECK(out.size() == 2 && out[0] == 1 && out[1] == 7);
    applied.assign(B, B + 3);
    memo0_stamp(nullptr, 0, n, stamp, epoch);                         // the empty set after a non-empty one: everything goes back
    memo0_restore_list(applied, stamp, epoch, out);
    CHECK(out.size() == 3 && out[0] == 9 && out[1] == 2 && out[2] == 4);
    memo0_stamp(B, 3, n, stamp, epoch);                               // the same set again: nothing to restore
    memo0_restore_list(applied, stamp, epoch, out);
    CHECK(out.empty());
    epoch = 0xffffffffu;                                              // the epoch is about to wrap: the stamps start over
    memo0_stamp(A, 4, n, stamp, epoch);
    CHECK(epoch == 1 && stamp[1] == 1 && stamp[2] == 0 && stamp[9] == 1);
    memo0_stamp(A, 4, 12, stamp, epoch);                              // another node count: the same
    CHECK(stamp.size() == 12 && epoch == 1);
    const int32_t bad[] = {-1, 12, 3};                                // (out-of-range ids are the evidence check's business: ignored here)
    memo0_stamp(bad, 3, 12, stamp, epoch);
    CHECK(stamp[3] == epoch);

    // ---- the constant part of sweep 0's residual
    const std::vector<double> cv = {0.5, 0.75, 0.5, 0.6, 0.75, 0.25};
    const std::vector<int32_t> order = {1, 4, 3, 0, 2, 5};            // descending contribution
    std::vector<uint32_t> st;
    uint32_t ep = 0;
    memo0_stamp(nullptr, 0, 6, st, ep);
    CHECK(memo0_const_residual(order, cv, st, ep) == 0.75);           // no evidence: the first
    const int32_t s1[] = {1};
    memo0_stamp(s1, 1, 6, st, ep);
    CHECK(memo0_const_residual(order, cv, st, ep) == 0.75);           // node 4 has the same
    const int32_t s2[] = {4, 1};
    memo0_stamp(s2, 2, 6, st, ep);
    CHECK(memo0_const_residual(order, cv, st, ep) == 0.6);
    const int32_t s3[] = {0, 1, 2, 3, 4};
    memo0_stamp(s3, 5, 6, st, ep);
    CHECK(memo0_const_residual(order, cv, st, ep) == 0.25);
    const int32_t s4[] = {0, 1, 2, 3, 4, 5};
    memo0_stamp(s4, 6, 6, st, ep);
    CHECK(memo0_const_residual(order, cv, st, ep) == 0.0);            // every node carries evidence: no constant part
    CHECK(!memo0_applies(run(true, true, false, 0, 1e-3, memo0_const_residual(order, cv, st, ep))));
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
