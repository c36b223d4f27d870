// test_batch_plan.cpp -- how a batch of evidence sets is planned (bayesiannetwork_amd/csrc/bn_engine_policy.cpp: which path takes
// it, whether it goes to the second, dense engine, the chunks of each path; bn_batch_stage.cpp: the layout of the evidence staging
// block), stand-alone: compiled with those two files alone by plain g++ (tests/test_cpp_batch_plan.py adds -fsanitize=address,undefined),
// no HIP and no library.  The expected values were worked out by hand from the rules as bn_engine_batch.cpp had them inline (900
// tiles, 0.9 x CUs / parts, 1..16 sets per DAG launch, balanced chunks of at most 4, 128 table entries, [nodes | offs | vals | meta]
// with the values 8-byte aligned and 8 meta words per set), not from running the functions.  "ok: ..." and exit status 0 on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bn_batch_stage.hpp"
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

// the four arguments every predicate takes, written by hand
struct Case {
    PathFacts f;
    ResidentShape r;
    PathOks ok;
    PathModes m;
    BatchDevice d{true, true};   // the one-workgroup state and a staging block exist
};
static bool small_w(const Case& c) { return batch_small_wanted(c.f, c.r, c.ok, c.m, c.d); }
static bool dag_w(const Case& c) { return batch_dag_wanted(c.f, c.r, c.ok, c.m, c.d); }
static bool mid_w(const Case& c) { return batch_mid_wanted(c.f, c.r, c.ok, c.m, c.d); }
static bool res_w(const Case& c) { return batch_resident_wanted(c.f, c.r, c.ok, c.m, c.d); }
static bool dense_w(const Case& c, int32_t n_sets) { return batch_wants_dense(c.f, c.r, c.ok, c.m, n_sets); }

// a network the register-resident DAG path takes under "dag" 1 when no one-workgroup plan exists: k = 4, lane groups, fits the chip
static Case dag_case() {
    Case c;
    c.ok.dag = true;
    c.f.dag.ok = true; c.f.dag.uniform4 = true; c.f.dag.has_groups = true; c.f.dag.fill = 1.0; c.f.dag.stream = false; c.f.dag.blocks = 64;
    return c;
}
// ... and one the several-workgroup item kernel takes: its plan exists and the resident tiles do not cover the network
static Case mid_case() {
    Case c;
    c.ok.mid = true;
    c.f.mid.ok = true; c.f.mid.parts = 8;
    return c;
}
static Case resident_case(int64_t tiles) {
    Case c;
    c.f.n_tiles = tiles;
    c.r.resident_ok = true; c.r.blocks = int((tiles + 7) / 8);
    return c;
}

static void predicates() {
    // one workgroup per set: eligible, "small" and "multisweep" not 0, the per-set state allocated, and not "dag" 2 on a DAG-eligible engine
    Case s; s.ok.small = true;
    CHECK(small_w(s));
    { Case c = s; c.ok.small = false; CHECK(!small_w(c)); }
    { Case c = s; c.m.small = 0; CHECK(!small_w(c)); }
    { Case c = s; c.m.small = 2; CHECK(small_w(c)); }
    { Case c = s; c.m.multisweep = 0; CHECK(!small_w(c)); }
    { Case c = s; c.m.multisweep = 2; CHECK(small_w(c)); }
    { Case c = s; c.d.small_state = false; CHECK(!small_w(c)); }
    { Case c = s; c.d.staged = false; CHECK(small_w(c)); }            // (it reads the block when there is one, else the tile buffers)
    { Case c = s; c.m.dag = 2; c.ok.dag = true; CHECK(!small_w(c)); }  // "dag" 2 with dag_ok: the DAG path goes first
    { Case c = s; c.m.dag = 2; c.ok.dag = false; CHECK(small_w(c)); }  // ... without: nothing to put in front
    { Case c = s; c.m.dag = 1; c.ok.dag = true; CHECK(small_w(c)); }
    { Case c = s; c.f.nranks = 2; CHECK(small_w(c)); }                 // (sharded engines are refused before any path is asked)

    // the register-resident DAG path: where the single-query policy applies it, with a staging block, on one rank, behind the one-workgroup path
    Case g = dag_case();
    CHECK(dag_w(g) && !small_w(g) && !mid_w(g) && !res_w(g));
    { Case c = g; c.d.staged = false; CHECK(!dag_w(c)); }
    { Case c = g; c.f.nranks = 2; CHECK(!dag_w(c)); }
    { Case c = g; c.m.dag = 0; CHECK(!dag_w(c)); }
    { Case c = g; c.m.multisweep = 0; CHECK(!dag_w(c)); }
    { Case c = g; c.m.multisweep = 2; CHECK(dag_w(c)); }
    { Case c = g; c.ok.dag = false; CHECK(!dag_w(c)); }
    { Case c = g; c.ok.dag = false; c.m.dag = 2; CHECK(!dag_w(c)); }
    { Case c = g; c.ok.small = true; CHECK(small_w(c) && !dag_w(c)); }                      // "dag" 1: a small network with lane groups stays on one workgroup
    { Case c = g; c.ok.small = true; c.m.dag = 2; CHECK(!small_w(c) && dag_w(c)); }         // "dag" 2: in front
    { Case c = g; c.ok.small = true; c.m.dag = 2; c.d.small_state = false; CHECK(dag_w(c)); }
    {   // "dag" 1 on a small network the single-query policy gives to the DAG path (three rounds, no groups): a batch still runs one workgroup per set
        Case c = g; c.ok.small = true; c.f.dag.has_groups = false; c.f.small.re = 3; c.f.small.mmax = 2;
        CHECK(dag_applies(c.f, c.r, c.ok, c.m) && small_w(c) && !dag_w(c));
        c.d.small_state = false;
        CHECK(!small_w(c) && dag_w(c));
        c.m.small = 0; c.d.small_state = true;
        CHECK(!small_w(c) && dag_w(c));
    }

    // the several-workgroup item kernel: where the single-query policy applies it, with a staging block, behind the one-workgroup path
    Case m = mid_case();
    CHECK(mid_w(m) && !small_w(m) && !dag_w(m) && !res_w(m));
    { Case c = m; c.d.staged = false; CHECK(!mid_w(c)); }
    { Case c = m; c.m.mid = 0; CHECK(!mid_w(c)); }
    { Case c = m; c.m.mid = 2; CHECK(mid_w(c)); }
    { Case c = m; c.m.multisweep = 0; CHECK(!mid_w(c)); }
    { Case c = m; c.ok.mid = false; CHECK(!mid_w(c)); }
    { Case c = m; c.ok.small = true; CHECK(small_w(c) && !mid_w(c)); }
    { Case c = m; c.ok.small = true; c.d.small_state = false; CHECK(mid_w(c)); }
    { Case c = m; c.f.nranks = 2; CHECK(mid_w(c)); }
    { Case c = m; c.r.resident_ok = true; CHECK(!mid_w(c)); }   // "mid" 1, covered by the tiles, one parent per node: stays on the tiles
    { Case c = m; c.r.resident_ok = true; c.m.mid = 2; CHECK(mid_w(c)); }

    // the resident tiles: eligible and "multisweep" 2, or "multisweep" 1 from 900 tiles up
    CHECK(!res_w(resident_case(899)));
    CHECK(res_w(resident_case(900)));
    CHECK(res_w(resident_case(1792)));
    { Case c = resident_case(899); c.m.multisweep = 2; CHECK(res_w(c)); }
    { Case c = resident_case(1); c.m.multisweep = 2; CHECK(res_w(c)); }
    { Case c = resident_case(1); CHECK(!res_w(c)); }                       // (one block pays for a single query, not for a batch)
    { Case c = resident_case(900); c.m.multisweep = 0; CHECK(!res_w(c)); }
    { Case c = resident_case(5000); c.m.multisweep = 0; CHECK(!res_w(c)); }
    { Case c = resident_case(900); c.r.resident_ok = false; CHECK(!res_w(c)); }
    { Case c = resident_case(900); c.r.resident_ok = false; c.m.multisweep = 2; CHECK(!res_w(c)); }
    { Case c = resident_case(900); c.ok.small = true; CHECK(small_w(c) && !res_w(c)); }
    { Case c = resident_case(900); c.ok.small = true; c.d.small_state = false; CHECK(res_w(c)); }
    { Case c = resident_case(900); c.d.staged = false; CHECK(res_w(c)); }  // (reads the tile buffers)
}

static void dense_rule() {
    // a layout built for one query's latency, one rank, two or more sets, and none of the paths on which the layout plays no part
    Case b; b.f.latency_rules_applied = true;
    CHECK(dense_w(b, 2) && dense_w(b, 256));
    CHECK(!dense_w(b, 1));
    { Case c = b; c.f.latency_rules_applied = false; CHECK(!dense_w(c, 2)); }
    { Case c = b; c.f.nranks = 2; CHECK(!dense_w(c, 2)); }
    // one workgroup per set: eligible with "small" and "multisweep" not 0 (whether its state is allocated plays no part here)
    { Case c = b; c.ok.small = true; CHECK(!dense_w(c, 2)); }
    { Case c = b; c.ok.small = true; c.d.small_state = false; CHECK(!dense_w(c, 2)); }
    { Case c = b; c.ok.small = true; c.m.small = 0; CHECK(dense_w(c, 2)); }
    { Case c = b; c.ok.small = true; c.m.multisweep = 0; CHECK(dense_w(c, 2)); }
    { Case c = b; c.ok.small = true; c.m.dag = 2; c.ok.dag = false; CHECK(!dense_w(c, 2)); }
    // the several-workgroup kernel and the DAG path where the single-query policy applies them
    { Case c = mid_case(); c.f.latency_rules_applied = true; CHECK(!dense_w(c, 2)); c.m.mid = 0; CHECK(dense_w(c, 2)); }
    { Case c = dag_case(); c.f.latency_rules_applied = true; CHECK(!dense_w(c, 2)); c.m.dag = 0; CHECK(dense_w(c, 2)); }
    { Case c = dag_case(); c.f.latency_rules_applied = true; c.m.multisweep = 0; CHECK(dense_w(c, 2)); }
    // the resident tiles DO depend on the layout
    { Case c = resident_case(900); c.f.latency_rules_applied = true; CHECK(dense_w(c, 2)); }

    // same bits: a node on another variant or lane-group width in the two layouts only matters beyond 128 table entries
    const NodeLayout a128{0, 1, 4, 128}, a129{0, 1, 4, 129}, skip{-1, 0, 0, 100000};
    {
        const NodeLayout own[] = {a128, a129}, same[] = {a128, a129};
        CHECK(dense_keeps_bits(own, 2, same, 2));
        CHECK(dense_keeps_bits(own, 0, same, 0));
    }
    {   // variant differs
        const NodeLayout own[] = {a128}, other[] = {{0, 2, 4, 128}};
        CHECK(dense_keeps_bits(own, 1, other, 1));
        const NodeLayout own9[] = {a129}, other9[] = {{0, 2, 4, 129}};
        CHECK(!dense_keeps_bits(own9, 1, other9, 1));
    }
    {   // G differs
        const NodeLayout own[] = {a128}, other[] = {{0, 1, 2, 128}};
        CHECK(dense_keeps_bits(own, 1, other, 1));
        const NodeLayout own9[] = {a128, a129}, other9[] = {a128, {3, 1, 2, 129}};
        CHECK(!dense_keeps_bits(own9, 2, other9, 2));
        const NodeLayout cls[] = {a129}, cls_only[] = {{7, 1, 4, 129}};   // another class NUMBER with the same variant and G: same bits
        CHECK(dense_keeps_bits(cls, 1, cls_only, 1));
    }
    {   // the OWN layout's table size counts
        const NodeLayout own[] = {{0, 1, 4, 128}}, other[] = {{0, 2, 2, 4096}};
        CHECK(dense_keeps_bits(own, 1, other, 1));
    }
    {   // a node either layout skips (class < 0) is not compared
        const NodeLayout own[] = {skip, a128}, other[] = {{0, 2, 2, 100000}, a128};
        CHECK(dense_keeps_bits(own, 2, other, 2));
        const NodeLayout own2[] = {{0, 1, 4, 100000}, a128}, other2[] = {skip, a128};
        CHECK(dense_keeps_bits(own2, 2, other2, 2));
        const NodeLayout own3[] = {{0, 1, 4, 100000}, a128}, other3[] = {{0, 2, 4, 100000}, a128};
        CHECK(!dense_keeps_bits(own3, 2, other3, 2));
    }
    {   // differing node counts: never the same network
        const NodeLayout own[] = {a128, a128}, other[] = {a128};
        CHECK(!dense_keeps_bits(own, 2, other, 1));
        CHECK(!dense_keeps_bits(own, 1, other, 0));
    }
}

static void chunks() {
    for (int32_t n = 1; n <= 256; ++n) {
        const std::vector<int32_t> c = resident_batch_chunks(n);
        CHECK(int32_t(c.size()) == (n + 3) / 4);
        int32_t sum = 0, lo = 1 << 30, hi = 0;
        for (int32_t x : c) { sum += x; lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
        CHECK(sum == n && hi <= 4 && lo >= 1 && hi - lo <= 1);
        for (size_t i = 1; i < c.size(); ++i) CHECK(c[i] <= c[i - 1]);   // the larger chunks first
    }
    CHECK((resident_batch_chunks(19) == std::vector<int32_t>{4, 4, 4, 4, 3}));
    CHECK((resident_batch_chunks(5) == std::vector<int32_t>{3, 2}));
    CHECK((resident_batch_chunks(4) == std::vector<int32_t>{4}));
    CHECK((resident_batch_chunks(9) == std::vector<int32_t>{3, 3, 3}));
    CHECK((resident_batch_chunks(1) == std::vector<int32_t>{1}));

    // max(1, min(B, 0.9 x CUs / parts)), integer arithmetic: 0.9 x 64 = 57, x 256 = 230, x 304 = 273
    CHECK(mid_sets_per_launch(64, 8, 256) == 7);
    CHECK(mid_sets_per_launch(64, 8, 5) == 5);
    CHECK(mid_sets_per_launch(64, 57, 3) == 1);
    CHECK(mid_sets_per_launch(64, 58, 3) == 1);      // the parts exceed 0.9 x CUs: still one set per launch
    CHECK(mid_sets_per_launch(64, 28, 3) == 2);
    CHECK(mid_sets_per_launch(64, 29, 3) == 1);
    CHECK(mid_sets_per_launch(256, 8, 100) == 28);
    CHECK(mid_sets_per_launch(256, 8, 28) == 28);
    CHECK(mid_sets_per_launch(256, 8, 27) == 27);
    CHECK(mid_sets_per_launch(256, 115, 4) == 2);
    CHECK(mid_sets_per_launch(256, 116, 4) == 1);
    CHECK(mid_sets_per_launch(256, 231, 4) == 1);
    CHECK(mid_sets_per_launch(256, 1, 256) == 230);
    CHECK(mid_sets_per_launch(256, 2, 1) == 1);
    CHECK(mid_sets_per_launch(304, 32, 256) == 8);
    CHECK(mid_sets_per_launch(304, 30, 256) == 9);
    CHECK(mid_sets_per_launch(304, 274, 2) == 1);

    CHECK(dag_sets_per_launch(0) == 16);     // not set
    CHECK(dag_sets_per_launch(1) == 1);
    CHECK(dag_sets_per_launch(8) == 8);
    CHECK(dag_sets_per_launch(16) == 16);
    CHECK(dag_sets_per_launch(17) == 16);
    CHECK(dag_sets_per_launch(-3) == 1);
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*, [0, n)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return uint32_t(((g_rng * 0x2545f4914f6cdd1dull) >> 33) % n);
}

// one batch: `empty` = every set without findings; null_off = the caller passes no offsets array (allowed only then)
static void staging_case(int32_t n_sets, bool empty, bool null_off) {
    std::vector<int32_t> ne(n_sets), node, off;
    std::vector<double> val;
    for (int32_t q = 0; q < n_sets; ++q) {
        ne[q] = empty ? 0 : int32_t(rnd(9));
        int32_t at = 0;
        off.push_back(0);
        for (int32_t i = 0; i < ne[q]; ++i) {
            const int32_t arity = 2 + int32_t(rnd(5));
            node.push_back(int32_t(rnd(100000)));
            for (int32_t s = 0; s < arity; ++s) val.push_back(double(rnd(1000)) / 8.0);
            at += arity;
            off.push_back(at);
        }
    }
    const int32_t* off_arg = null_off ? nullptr : off.data();
    const bn_stage::BatchLayout l = bn_stage::layout_of(n_sets, ne.data(), off_arg);
    // the prefix arrays by a naive loop
    CHECK(l.n_sets == n_sets && int32_t(l.node_at.size()) == n_sets + 1 && l.off_at.size() == l.node_at.size() && l.val_at.size() == l.node_at.size());
    int64_t nn = 0, no = 0, nv = 0;
    for (int32_t q = 0; q < n_sets; ++q) {
        CHECK(l.node_at[q] == nn && l.off_at[q] == no && l.val_at[q] == nv);
        nn += ne[q];
        nv += ne[q] > 0 ? off[size_t(no + ne[q])] : 0;
        no += ne[q] + 1;
    }
    CHECK(l.node_at[n_sets] == nn && l.off_at[n_sets] == no && l.val_at[n_sets] == nv);
    CHECK(nn == int64_t(node.size()) && no == int64_t(off.size()) && nv == int64_t(val.size()));
    // the four parts
    CHECK(l.b_node == 0 && l.b_off == size_t(nn) * 4);
    CHECK(l.b_val % 8 == 0 && l.b_val >= l.b_off + size_t(no) * 4 && l.b_val < l.b_off + size_t(no) * 4 + 8);
    CHECK(l.b_meta == l.b_val + size_t(nv) * 8);
    CHECK(l.bytes == l.b_meta + 32 * size_t(n_sets));
    // fill against a block assembled field by field (what fill leaves alone -- padding, the offsets of a null ev_off -- keeps the pattern)
    std::vector<double> got_store(l.bytes / 8 + 1), want_store(l.bytes / 8 + 1);   // (8-byte aligned storage)
    char* got = reinterpret_cast<char*>(got_store.data());
    char* want = reinterpret_cast<char*>(want_store.data());
    std::memset(got, 0xAB, l.bytes);
    std::memset(want, 0xAB, l.bytes);
    for (size_t i = 0; i < node.size(); ++i) std::memcpy(want + 4 * i, &node[i], 4);
    if (!null_off) for (size_t i = 0; i < off.size(); ++i) std::memcpy(want + l.b_off + 4 * i, &off[i], 4);
    for (size_t i = 0; i < val.size(); ++i) std::memcpy(want + l.b_val + 8 * i, &val[i], 8);
    {
        int32_t first_node = 0, first_off = 0, first_val = 0;
        for (int32_t q = 0; q < n_sets; ++q) {
            const int32_t values = ne[q] > 0 ? off[size_t(first_off + ne[q])] : 0;
            const int32_t words[8] = {ne[q], first_node, first_off, first_val, values, 0, 0, 0};
            std::memcpy(want + l.b_meta + 32 * size_t(q), words, 32);
            first_node += ne[q]; first_off += ne[q] + 1; first_val += values;
        }
    }
    l.fill(got, node.data(), off_arg, val.data());
    CHECK(std::memcmp(got, want, l.bytes) == 0);
    CHECK(reinterpret_cast<char*>(l.meta(got)) == got + l.b_meta);
    // set_view(q): the set's count and its first entries
    int32_t first_node = 0, first_off = 0, first_val = 0;
    for (int32_t q = 0; q < n_sets; ++q) {
        const bn_stage::SetView v = l.set_view(got, q);
        CHECK(v.ne == ne[q]);
        CHECK(reinterpret_cast<char*>(v.node) == got + 4 * size_t(first_node));
        CHECK(reinterpret_cast<char*>(v.off) == got + l.b_off + 4 * size_t(first_off));
        CHECK(reinterpret_cast<char*>(v.val) == got + l.b_val + 8 * size_t(first_val));
        if (ne[q] > 0) {
            CHECK(v.node[0] == node[size_t(first_node)] && v.off[0] == 0 && v.val[0] == val[size_t(first_val)]);
            CHECK(v.off[ne[q]] == off[size_t(first_off + ne[q])]);
        }
        first_node += ne[q]; first_off += ne[q] + 1;
        first_val += ne[q] > 0 ? off[size_t(first_off - 1)] : 0;
    }
}

static void staging() {
    for (int i = 0; i < 300; ++i) staging_case(1 + int32_t(rnd(256)), false, false);
    for (int32_t n : {1, 2, 3, 4, 5, 255, 256}) staging_case(n, false, false);
    for (int32_t n : {1, 2, 7, 256}) {
        staging_case(n, true, false);   // every set empty, offsets given (one 0 per set)
        staging_case(n, true, true);    // ... and not given
    }
    {   // by hand: two sets, {node 5: (0.25, 0.75)} and {} -- nodes [5], offs [0, 2 | 0], vals at byte 16, meta at 32, 96 bytes
        const int32_t ne[] = {1, 0}, node[] = {5}, off[] = {0, 2, 0};
        const double val[] = {0.25, 0.75};
        const bn_stage::BatchLayout l = bn_stage::layout_of(2, ne, off);
        CHECK(l.b_node == 0 && l.b_off == 4 && l.b_val == 16 && l.b_meta == 32 && l.bytes == 96);
        CHECK(l.node_at[1] == 1 && l.node_at[2] == 1 && l.off_at[1] == 2 && l.off_at[2] == 3 && l.val_at[1] == 2 && l.val_at[2] == 2);
        double store[12];
        char* blk = reinterpret_cast<char*>(store);
        l.fill(blk, node, off, val);
        CHECK(l.meta(blk)[0] == 1 && l.meta(blk)[4] == 2 && l.meta(blk)[8] == 0 && l.meta(blk)[9] == 1 && l.meta(blk)[10] == 2 && l.meta(blk)[11] == 2 && l.meta(blk)[12] == 0);
        CHECK(l.set_view(blk, 0).val[1] == 0.75 && l.set_view(blk, 1).ne == 0);
    }
}

int main() {
    predicates();
    dense_rule();
    chunks();
    staging();
    std::printf("ok: %ld checks of the batch policy, the chunk arithmetic and the staging layout\n", g_checks);
    return 0;
}
