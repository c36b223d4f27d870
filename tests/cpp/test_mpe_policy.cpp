// test_mpe_policy.cpp -- which form of the max-product kernels runs a network (bn_policy::mpe_form, bayesiannetwork_amd/csrc/
// bn_engine_policy.cpp), stand-alone: compiled together with bn_engine_policy.cpp by plain g++ (tests/test_cpp_mpe_policy.py also
// builds it with -fsanitize=address,undefined), no HIP and no library.  The facts are written by hand, on both sides of each
// threshold.  The expected values come from the rule as the issue states it -- the one-workgroup form when the small plan is ok, else
// the several-workgroup form when the mid plan is ok and its parts fit 0.9 x CUs (integer arithmetic: parts <= CUs * 9 / 10; CU count 0
// = unknown, fits), else none; a forced form only where the network is eligible for it -- not from running the function.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <cstdio>
#include <cstdlib>

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

static PathFacts facts(bool small_ok, bool mid_ok, int32_t parts) {
    PathFacts f;
    f.small.ok = small_ok;
    f.mid.ok = mid_ok;
    f.mid.parts = parts;
    return f;
}

int main() {
    // ---- small plan ok / not ok
    CHECK(mpe_form(facts(true, false, 0), 256, 0) == 1);
    CHECK(mpe_form(facts(true, true, 2), 256, 0) == 1);      // both plans: the one-workgroup form goes first
    CHECK(mpe_form(facts(false, true, 2), 256, 0) == 2);
    CHECK(mpe_form(facts(false, false, 0), 256, 0) == 0);    // neither plan (more than 8 parents, beyond 224 parts)
    // ---- mid plan fits 0.9 x CUs / does not: 256 CUs -> 230, 64 -> 57, 304 -> 273
    CHECK(mpe_form(facts(false, true, 230), 256, 0) == 2);
    CHECK(mpe_form(facts(false, true, 231), 256, 0) == 0);
    CHECK(mpe_form(facts(false, true, 57), 64, 0) == 2);
    CHECK(mpe_form(facts(false, true, 58), 64, 0) == 0);
    CHECK(mpe_form(facts(false, true, 224), 304, 0) == 2);   // the planner's own limit of 224 parts fits 304 CUs
    CHECK(mpe_form(facts(false, true, 273), 304, 0) == 2);
    CHECK(mpe_form(facts(false, true, 274), 304, 0) == 0);
    CHECK(mpe_form(facts(false, true, 224), 0, 0) == 2);     // CU count unknown (no device): fits
    CHECK(mpe_form(facts(true, true, 231), 256, 0) == 1);    // the one-workgroup form does not care
    // ---- forced forms: that form where eligible, else none -- never the other one
    CHECK(mpe_form(facts(true, true, 2), 256, 1) == 1);
    CHECK(mpe_form(facts(true, true, 2), 256, 2) == 2);
    CHECK(mpe_form(facts(true, false, 0), 256, 2) == 0);
    CHECK(mpe_form(facts(false, true, 2), 256, 1) == 0);
    CHECK(mpe_form(facts(true, true, 231), 256, 2) == 0);    // forced, but the parts do not fit
    CHECK(mpe_form(facts(true, true, 230), 256, 2) == 2);
    CHECK(mpe_form(facts(false, false, 0), 256, 1) == 0);
    CHECK(mpe_form(facts(false, false, 0), 256, 2) == 0);
    std::printf("ok: %ld checks\n", g_checks);
    return 0;
}
