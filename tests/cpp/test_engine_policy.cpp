// test_engine_policy.cpp -- which kernel runs a query (bayesiannetwork_amd/csrc/bn_engine_policy.cpp), stand-alone: compiled together
// with bn_engine_policy.cpp by plain g++ (tests/test_cpp_engine_policy.py adds -fsanitize=address,undefined), no HIP and no library.
// The facts are written by hand and put on both sides of every threshold of the resident launch shape (at 256, 64 and 304 CUs) and
// of the path predicates.  The expected values were worked out from the rules as the engine had them inline before they became
// functions (0.9 x CUs caps, rounding to 8 blocks, 600 tiles, 128 nodes, 580 000 staged terms, fill 0.25), not from running the
// functions.  Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
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

// a single engine whose tiles the resident kernel runs: uniform, two parents, two children, k = 4, with a neighbour table
static PathFacts tiles(int64_t n_tiles, int32_t nranks = 1) {
    PathFacts f;
    f.nranks = nranks;
    f.n_tiles = n_tiles;
    f.all_uniform = true;
    f.tile_cmax = 2;
    f.tile_m = 2;
    f.tile_kv = 4;
    f.rec_total_doubles = 1 << 20;
    f.nbr_empty = false;
    f.kmax = 4;
    return f;
}

static void expect_shape(const PathFacts& f, int n_cus, int forced, int waves, int blocks, bool ok, int line) {
    const ResidentShape r = plan_resident(f, n_cus, forced);
    ++g_checks;
    if (r.waves != waves || r.blocks != blocks || r.resident_ok != ok) {
        std::printf("FAILED %s:%d: %lld tiles, %d ranks, %d CUs, forced %d: waves %d blocks %d ok %d, expected %d %d %d\n", __FILE__, line,
                    (long long)f.n_tiles, f.nranks, n_cus, forced, r.waves, r.blocks, int(r.resident_ok), waves, blocks, int(ok));
        std::exit(1);
    }
}
#define SHAPE(f, cus, forced, waves, blocks, ok) expect_shape(f, cus, forced, waves, blocks, ok, __LINE__)

static void resident_rule_256() {
    // 0.9 x 256 = 230: the tile blocks, rounded to a multiple of 8 when there is more than one, + the service block must fit
    SHAPE(tiles(898), 256, 0, 8, 120, true);    // 225 blocks of four round to 232: too many -> 8 waves, 113 -> 120 blocks
    SHAPE(tiles(897), 256, 0, 8, 120, true);    // 225 -> 232 as well
    SHAPE(tiles(896), 256, 0, 4, 224, true);    // one rounding step below: 224 blocks of four, 225 <= 230
    SHAPE(tiles(8), 256, 0, 8, 1, true);        // four waves only with MORE than 8 tiles
    SHAPE(tiles(9), 256, 0, 4, 8, true);        // 3 blocks round to 8
    SHAPE(tiles(1), 256, 0, 8, 1, true);
    SHAPE(tiles(0), 256, 0, 8, 0, false);       // no tile: nothing to run
    // BN_RESIDENT_WAVES: 8 always, 4 and 2 only where the blocks fit (2: more than 2 tiles)
    SHAPE(tiles(100), 256, 0, 4, 32, true);
    SHAPE(tiles(100), 256, 8, 8, 16, true);
    SHAPE(tiles(898), 256, 4, 8, 120, true);    // 232 blocks do not fit: not honoured
    SHAPE(tiles(8), 256, 4, 4, 8, true);        // honoured below the default's 9 tiles
    SHAPE(tiles(100), 256, 2, 2, 56, true);
    SHAPE(tiles(2), 256, 2, 8, 1, true);
    SHAPE(tiles(3), 256, 2, 2, 8, true);
    SHAPE(tiles(500), 256, 2, 4, 128, true);    // 250 -> 256 blocks of two: too many -> the default (125 -> 128 of four)
    SHAPE(tiles(448), 256, 2, 2, 224, true);
    SHAPE(tiles(100), 256, 3, 4, 32, true);     // any other value: ignored
    SHAPE(tiles(100), 256, 16, 4, 32, true);
    // blocks + 1 <= 230 at 8 waves
    SHAPE(tiles(1792), 256, 0, 8, 224, true);
    SHAPE(tiles(1793), 256, 0, 8, 232, false);  // 225 -> 232
    // a sharded rank is not rounded to 8 (and is never resident_ok: it exchanges in the kernel, shard_shapes_ok)
    SHAPE(tiles(100, 2), 256, 0, 4, 25, false);
    CHECK(plan_resident(tiles(100, 2), 256, 0).shard_shapes_ok);
    SHAPE(tiles(916, 2), 256, 0, 4, 229, false);   // 229 + 1 <= 230
    SHAPE(tiles(917, 2), 256, 0, 8, 115, false);   // 230 blocks of four: no
    SHAPE(tiles(1832, 2), 256, 0, 8, 229, false);
    CHECK(plan_resident(tiles(1832, 2), 256, 0).shard_shapes_ok);
    CHECK(!plan_resident(tiles(1833, 2), 256, 0).shard_shapes_ok);   // 230 + 1 > 230
    CHECK(plan_resident(tiles(100, 16), 256, 0).shard_shapes_ok);    // kMaxRanks
    CHECK(!plan_resident(tiles(100, 17), 256, 0).shard_shapes_ok);
    CHECK(!plan_resident(tiles(100), 256, 0).shard_shapes_ok);
    // 32-bit byte offsets into a record buffer: rec_total_doubles * 8 < 2^31
    PathFacts f = tiles(100);
    f.rec_total_doubles = (int64_t(1) << 28) - 1;
    CHECK(plan_resident(f, 256, 0).resident_ok);
    f.rec_total_doubles = int64_t(1) << 28;
    CHECK(!plan_resident(f, 256, 0).resident_ok);
    f.nranks = 2;
    CHECK(!plan_resident(f, 256, 0).shard_shapes_ok);
    // the tiles' shapes
    f = tiles(100); f.all_uniform = false; CHECK(!plan_resident(f, 256, 0).resident_ok);
    f = tiles(100); f.tile_cmax = 8; CHECK(plan_resident(f, 256, 0).resident_ok);
    f = tiles(100); f.tile_cmax = 9; CHECK(!plan_resident(f, 256, 0).resident_ok);
    f = tiles(100); f.tile_m = 3; CHECK(!plan_resident(f, 256, 0).resident_ok);
    f = tiles(100); f.any_in_ref = true; CHECK(!plan_resident(f, 256, 0).resident_ok);
    f = tiles(100, 2); f.any_in_ref = true; CHECK(plan_resident(f, 256, 0).shard_shapes_ok);   // (a shard's tiles have them)
    // lean: the common arity where no tile has more than two children
    CHECK(plan_resident(tiles(100), 256, 0).lean == 4);
    CHECK(plan_resident(tiles(100, 2), 256, 0).lean == 4);
    f = tiles(100); f.tile_kv = 2; CHECK(plan_resident(f, 256, 0).lean == 2);
    f = tiles(100); f.tile_kv = 0; CHECK(plan_resident(f, 256, 0).lean == 0);   // mixed
    f = tiles(100); f.tile_cmax = 3; f.any_cmax_gt2 = true; CHECK(plan_resident(f, 256, 0).lean == 0);
    f = tiles(100); f.tile_m = 3; CHECK(plan_resident(f, 256, 0).lean == 0);    // not eligible at all
    // the dataflow form: eligible, more than one block, a neighbour table
    CHECK(plan_resident(tiles(9), 256, 0).flow_ok);
    CHECK(!plan_resident(tiles(8), 256, 0).flow_ok);
    f = tiles(9); f.nbr_empty = true; CHECK(!plan_resident(f, 256, 0).flow_ok);
    CHECK(!plan_resident(tiles(1793), 256, 0).flow_ok);
    CHECK(!plan_resident(tiles(100, 2), 256, 0).flow_ok);
}

static void resident_rule_other_devices() {
    // 64 CUs: 0.9 x 64 = 57
    SHAPE(tiles(898), 64, 0, 8, 120, false);
    SHAPE(tiles(224), 64, 0, 4, 56, true);
    SHAPE(tiles(225), 64, 0, 8, 32, true);      // 57 -> 64 blocks of four: too many
    SHAPE(tiles(448), 64, 0, 8, 56, true);
    SHAPE(tiles(449), 64, 0, 8, 64, false);
    SHAPE(tiles(9), 64, 0, 4, 8, true);
    SHAPE(tiles(224), 64, 2, 4, 56, true);      // 112 blocks of two: no
    SHAPE(tiles(112), 64, 2, 2, 56, true);
    SHAPE(tiles(456, 2), 64, 0, 8, 57, false);
    CHECK(!plan_resident(tiles(456, 2), 64, 0).shard_shapes_ok);   // 57 + 1 > 57
    CHECK(plan_resident(tiles(448, 2), 64, 0).shard_shapes_ok);
    // 304 CUs: 0.9 x 304 = 273, so kResidentMaxBlocks = 256 is the limit
    SHAPE(tiles(898), 304, 0, 4, 232, true);
    SHAPE(tiles(1024), 304, 0, 4, 256, true);
    SHAPE(tiles(1025), 304, 0, 8, 136, true);   // 257 -> 264 blocks of four > 256
    SHAPE(tiles(2048), 304, 0, 8, 256, true);
    SHAPE(tiles(2049), 304, 0, 8, 264, false);
    SHAPE(tiles(2049, 2), 304, 0, 8, 257, false);
    CHECK(plan_resident(tiles(2048, 2), 304, 0).shard_shapes_ok);
    CHECK(!plan_resident(tiles(2049, 2), 304, 0).shard_shapes_ok);
    CHECK(plan_resident(tiles(2048), 304, 0).flow_ok);
    // the two other caps
    PathFacts f;
    f.mid.ok = true;
    f.mid.parts = 230; CHECK(mid_fits(f, 256));
    f.mid.parts = 231; CHECK(!mid_fits(f, 256));
    f.mid.parts = 57; CHECK(mid_fits(f, 64)); CHECK(mid_fits(f, 0));   // (0: no device known)
    f.mid.parts = 58; CHECK(!mid_fits(f, 64)); CHECK(mid_fits(f, 304));
    CHECK(dag_cap(256) == 224 && dag_cap(64) == 56 && dag_cap(304) == 272 && dag_cap(8) == 0);
}

static ResidentShape shape_of(int waves, int blocks, bool ok) {
    ResidentShape r;
    r.waves = waves; r.blocks = blocks; r.resident_ok = ok;
    return r;
}

static void resident_and_small() {
    const PathOks none{};
    PathModes m;
    // 600 tiles with 8 waves per block; one block and 4 waves pay at any size
    CHECK(!resident_wanted(tiles(599), shape_of(8, 80, true), none, m));
    CHECK(resident_wanted(tiles(600), shape_of(8, 80, true), none, m));
    CHECK(resident_wanted(tiles(5), shape_of(8, 1, true), none, m));
    CHECK(resident_wanted(tiles(599), shape_of(4, 152, true), none, m));
    CHECK(!resident_wanted(tiles(600), shape_of(8, 80, false), none, m));
    m.multisweep = 2;
    CHECK(resident_wanted(tiles(599), shape_of(8, 80, true), none, m));
    CHECK(!resident_wanted(tiles(599), shape_of(8, 80, false), none, m));
    m.multisweep = 0;
    CHECK(!resident_wanted(tiles(600), shape_of(8, 80, true), none, m));
    CHECK(!resident_wanted(tiles(5), shape_of(8, 1, true), none, m));
    // shards: the in-kernel exchange wherever the peers are mapped
    PathOks mapped{};
    mapped.shard_flow = true;
    m.multisweep = 1;
    CHECK(resident_wanted(tiles(100, 2), shape_of(8, 13, false), mapped, m));
    CHECK(!resident_wanted(tiles(100, 2), shape_of(8, 13, false), none, m));
    m.multisweep = 0;
    CHECK(!resident_wanted(tiles(100, 2), shape_of(8, 13, false), mapped, m));

    // the one-workgroup path: everywhere but where the resident tiles run the network in ONE block and were measured faster
    PathOks ok{};
    ok.small = true;
    m = PathModes();
    PathFacts f = tiles(4);
    f.small = {true, 128, 1, 1, 1, 1};   // ok, n, re, rb, rc, mmax: a chain
    const ResidentShape one = shape_of(8, 1, true), two = shape_of(4, 8, true), not_res = shape_of(8, 1, false);
    CHECK(small_wanted(f, one, ok, m));
    f.small.n = 129; CHECK(!small_wanted(f, one, ok, m));
    CHECK(small_wanted(f, two, ok, m));        // more than one block
    CHECK(small_wanted(f, not_res, ok, m));    // not resident-eligible
    f.small.n = 100; f.small.re = 2; CHECK(!small_wanted(f, one, ok, m));
    f.small.mmax = 2; CHECK(small_wanted(f, one, ok, m));                      // two parents: whatever the rounds and the size
    f.small.n = 500; f.small.re = 4; CHECK(small_wanted(f, one, ok, m));
    f.small.rb = 2; CHECK(!small_wanted(f, one, ok, m));
    f.small.rb = 1; f.small.rc = 2; CHECK(!small_wanted(f, one, ok, m));
    f.small.rc = 1; CHECK(small_wanted(f, one, ok, m));
    f.small.rb = 2;
    m.small = 2; CHECK(small_wanted(f, one, ok, m));
    m.small = 0; CHECK(!small_wanted(f, two, ok, m));
    m.small = 1; CHECK(!small_wanted(f, two, none, m));   // tables not on the device
    m.small = 2; CHECK(!small_wanted(f, two, none, m));
    m.multisweep = 0; CHECK(!small_wanted(f, two, ok, m));
}

static void mid_path() {
    PathOks ok{};
    ok.mid = true;
    PathModes m;
    PathFacts f = tiles(200);
    f.mid.ok = true; f.mid.parts = 8; f.mid.mmax = 2; f.mid.est_total = 580000;
    const ResidentShape res = shape_of(4, 56, true), not_res = shape_of(4, 56, false);
    CHECK(mid_applies(f, res, ok, m));
    f.mid.est_total = 580001; CHECK(!mid_applies(f, res, ok, m));
    CHECK(mid_applies(f, not_res, ok, m));     // nothing else takes the network
    m.mid = 2; CHECK(mid_applies(f, res, ok, m));
    m.mid = 0; CHECK(!mid_applies(f, not_res, ok, m));
    m.mid = 1;
    f.mid.est_total = 1000;
    f.kmax = 3; CHECK(!mid_applies(f, res, ok, m));
    f.kmax = 4; CHECK(mid_applies(f, res, ok, m));
    f.kmax = 5; CHECK(mid_applies(f, res, ok, m));
    f.mid.mmax = 1; CHECK(!mid_applies(f, res, ok, m));
    f.mid.mmax = 2; CHECK(mid_applies(f, res, ok, m));
    m.multisweep = 0; CHECK(!mid_applies(f, res, ok, m)); CHECK(!mid_applies(f, not_res, ok, m));
    m.multisweep = 1; m.mid = 2; CHECK(!mid_applies(f, res, PathOks{}, m));
}

static void dag_path() {
    PathOks dag{}, both{};
    dag.dag = true;
    both.dag = true; both.small = true;
    PathModes m;
    const ResidentShape one = shape_of(8, 1, true), many = shape_of(4, 56, true);
    PathFacts f = tiles(200);
    f.dag.ok = true; f.dag.uniform4 = true; f.dag.has_groups = false; f.dag.fill = 1.0; f.dag.stream = false; f.dag.blocks = 25;
    f.small = {true, 64, 3, 1, 1, 2};
    // line by line
    CHECK(dag_applies(f, many, dag, m));
    CHECK(!dag_applies(f, many, PathOks{}, m));                         // not set up on the device
    m.multisweep = 0; CHECK(!dag_applies(f, many, dag, m)); m.multisweep = 1;
    m.dag = 0; CHECK(!dag_applies(f, many, dag, m));
    m.dag = 2; f.small.re = 1; f.dag.stream = true; f.dag.fill = 0.01; CHECK(dag_applies(f, one, both, m));   // forced: nothing else is asked
    m.dag = 1; f.dag.stream = false; f.dag.fill = 1.0;
    f.small.re = 2; CHECK(!dag_applies(f, many, both, m));              // up to two rounds of entry items: the one-workgroup path
    CHECK(dag_applies(f, many, dag, m));                                //   ... where it is set up
    f.small.re = 3; CHECK(dag_applies(f, many, both, m));
    f.dag.has_groups = true; CHECK(!dag_applies(f, many, both, m));     // >= 3 parents on a small network: the two paths' bits differ
    CHECK(dag_applies(f, many, dag, m));
    f.dag.has_groups = false;
    f.small.mmax = 1; CHECK(!dag_applies(f, one, both, m));             // chains and trees the resident tiles run in one block
    CHECK(dag_applies(f, many, both, m));
    CHECK(dag_applies(f, shape_of(8, 1, false), both, m));
    CHECK(dag_applies(f, one, dag, m));
    f.small.mmax = 2; CHECK(dag_applies(f, one, both, m));
    // padded form without lane groups: not below a quarter real
    f.dag.uniform4 = false;
    f.dag.fill = 0.2499; CHECK(!dag_applies(f, many, dag, m));
    f.dag.fill = 0.25; CHECK(dag_applies(f, many, dag, m));
    f.dag.fill = 0.2499; f.dag.has_groups = true; CHECK(dag_applies(f, many, dag, m));   // lane groups: this rule does not apply
    f.dag.uniform4 = true; f.dag.has_groups = false; CHECK(dag_applies(f, many, dag, m)); // (a k = 4 network is all real anyway)
    // stream form: not below a quarter real, whatever the parent counts
    f.dag.uniform4 = false; f.dag.has_groups = true; f.dag.stream = true;
    f.dag.fill = 0.2499; CHECK(!dag_applies(f, many, dag, m));
    f.dag.fill = 0.25; CHECK(dag_applies(f, many, dag, m));
    // lane groups take the stream form, nodes of <= 2 parents do not
    f.dag.uniform4 = true; f.dag.fill = 1.0;
    CHECK(dag_applies(f, many, dag, m));
    f.dag.has_groups = false; CHECK(!dag_applies(f, many, dag, m));
    f.dag.stream = false; CHECK(dag_applies(f, many, dag, m));

    // ahead of the one-workgroup path, or behind it
    f.small = {true, 64, 3, 1, 1, 2};
    m = PathModes();
    CHECK(dag_first_wanted(f, many, both, m) && !dag_later_wanted(f, many, both, m));    // a small network of three rounds
    CHECK(!dag_first_wanted(f, many, dag, m) && dag_later_wanted(f, many, dag, m));      // no one-workgroup path: its usual place
    m.small = 2;
    CHECK(!dag_first_wanted(f, many, both, m) && dag_later_wanted(f, many, both, m));    // "small" 2 goes first
    m.dag = 2;
    CHECK(dag_first_wanted(f, many, both, m) && !dag_later_wanted(f, many, both, m));    // ... unless "dag" 2 as well
    m.small = 1;
    CHECK(dag_first_wanted(f, many, dag, m) && !dag_later_wanted(f, many, dag, m));
    f.small.re = 1; m.dag = 1;
    CHECK(!dag_first_wanted(f, many, both, m) && !dag_later_wanted(f, many, both, m));   // does not apply: neither
    m.dag = 0; f.small.re = 3;
    CHECK(!dag_first_wanted(f, many, both, m) && !dag_later_wanted(f, many, both, m));
}

static void multisweep_off() {
    PathOks all{};
    all.small = all.mid = all.dag = all.shard_flow = true;
    PathFacts f = tiles(700);
    f.small = {true, 64, 3, 1, 1, 2};
    f.mid.ok = true; f.mid.parts = 8; f.mid.mmax = 2; f.mid.est_total = 1000;
    f.dag.ok = true; f.dag.uniform4 = true; f.dag.fill = 1.0;
    const ResidentShape r = shape_of(8, 88, true);
    for (int forced = 0; forced <= 2; ++forced) {
        PathModes m;
        m.multisweep = 0; m.small = m.mid = m.dag = forced;
        CHECK(!resident_wanted(f, r, all, m) && !small_wanted(f, r, all, m) && !mid_applies(f, r, all, m) && !dag_applies(f, r, all, m) &&
              !dag_first_wanted(f, r, all, m) && !dag_later_wanted(f, r, all, m));
    }
    PathFacts sh = tiles(100, 2);
    PathModes m;
    m.multisweep = 0;
    CHECK(!resident_wanted(sh, r, all, m));
    m.multisweep = 1; m.small = m.mid = m.dag = 1;   // (the same facts under the default options: every path wants the network)
    CHECK(resident_wanted(f, r, all, m) && small_wanted(f, r, all, m) && mid_applies(f, r, all, m) && dag_first_wanted(f, r, all, m));
}

int main() {
    resident_rule_256();
    resident_rule_other_devices();
    resident_and_small();
    mid_path();
    dag_path();
    multisweep_off();
    std::printf("ok: %ld expectations on the resident launch shape and the path predicates\n", g_checks);
    return 0;
}
