// bn_engine_memo.cpp -- the first-sweep image of the resident path (option "memo0"; bn_device.hpp Memo0Args, bn_kernels.hip memo0_node).
// Sweep 0 of a run reads no message: what a node's lane leaves behind depends on the node's CPT and its own evidence alone.  The
// engine keeps that state -- records and node vectors in the layout of rec1 / node1, the buffers sweep 1 reads -- computed ONCE per
// CPT image for the network without evidence; the launch that applies an evidence set (flush_evidence) recomputes the slots of the
// set's nodes and of the nodes the set drops, O(evidence) work in the same single launch; a run of the grid-barrier form then starts
// at sweep 1 (bn_engine_paths.cpp run_resident).  The decisions are pure host functions (bn_engine_policy.hpp memo0_*).
// The second-sweep image (option "memo1"; Memo1Args, memo_step_node) carries the argument one sweep further: what sweep 1 leaves at a
// node depends on the evidence of its closed neighbourhood alone.  It is built from the PRISTINE first-sweep image -- right after that
// one's build launch, before the evidence in force is patched into it, with the marks ignored -- and a launch queued behind the
// first-sweep patch recomputes the closed neighbourhoods of the set's nodes and of the nodes it drops; a run then starts at sweep 2.
#include "bn_engine_internal.hpp"

#include <numeric>

bool bn_eng::memo0_possible(const bn_engine* e) {
    return e->memo.enabled != 0 && e->shape.resident_ok && e->plan.nranks == 1 && e->plan.n > 0;
}

// Lanes per node of a patch launch, as a shift (Memo0Args::spread).  A node's table is 32 scattered lines; measured on the 316 x 316
// grid with 2 x 998 nodes per launch (EXPERIMENTS R19.4), us per launch: 14.6 at one node per lane, 11.6 at one per 4 lanes, 14.7
// at one per 16, 33.3 at one per 64 (bp_evidence_kernel: 11.7).  Large sets fill the chip at one node per lane (not measured).
// BN_MEMO0_SPREAD forces a value (experiments).
static int memo0_spread(int32_t work) {
    static const int forced = std::getenv("BN_MEMO0_SPREAD") ? std::max(0, std::min(std::atoi(std::getenv("BN_MEMO0_SPREAD")), 6)) : -1;
    if (forced >= 0) return forced;
    return work <= 8192 ? 2 : 0;
}

void bn_eng::memo0_invalidate(bn_engine* e) {
    e->memo.valid = false;
    e->memo.applied.clear();
    e->memo1.built = false;   // (built from the first-sweep image: both go together)
    e->memo1.holds = false;
    e->memo1.applied.clear();
}

// Lanes per thread of the second-sweep patch, as a shift: as memo0_spread (a node's table is 32 scattered lines).  BN_MEMO1_SPREAD
// forces a value (experiments).
static int memo1_spread(int64_t work) {
    static const int forced = std::getenv("BN_MEMO1_SPREAD") ? std::max(0, std::min(std::atoi(std::getenv("BN_MEMO1_SPREAD")), 6)) : -1;
    if (forced >= 0) return forced;
    return work <= 8192 ? 2 : 0;
}

// The second-sweep image for the evidence in force, behind the first-sweep patch of the same set (whose stamps say what the set is):
// one launch over the closed neighbourhoods of the set's nodes and of the nodes this image held and the set drops -- or none, when
// the set is over the work limit or arrives with its single run and that was measured not to pay (bn_policy::memo1_plan_set); the
// image then keeps its own list of what it holds, and runs start at sweep 1 until a set patches again.
static int memo1_patch(bn_engine* e) {
    bn_engine::Memo1& m1 = e->memo1;
    const bn_engine::Memo0& m = e->memo;
    m1.holds = false;
    if (!m1.built) return BN_OK;
    const int32_t ne = e->ev_ne;
    const int32_t* nodes = ne > 0 ? reinterpret_cast<const int32_t*>(e->h_ev.get()) : nullptr;
    const bool wanted = !(e->ev_one_shot && m1.oneshot == 0);
    const bn_policy::Memo1Plan plan = bn_policy::memo1_plan_set(nodes, ne, m.stamp, m.epoch, wanted, m1.max_degree, m1.limit, m1.applied, m1.list);
    if (!plan.holds) return BN_OK;
    m1.seed = bn_policy::memo1_seed(m1.order, m1.cv, m1.adj_off, m1.adj, m.stamp, m.epoch);
    if (!plan.patch) {   // nothing to apply, nothing to restore: the pristine image, sweep 1's residual is the constant word
        m1.word = 2;
        m1.holds = true;
        return BN_OK;
    }
    std::memcpy(m1.h_list.get(), m1.list.data(), m1.list.size() * sizeof(int32_t));
    unsigned long long seed = 0;
    std::memcpy(&seed, &m1.seed, sizeof seed);
    const int32_t width = 1 + m1.max_degree;
    Memo1Args a{buffers_of(e), m.d_rec, m.d_node, m1.d_rec, m1.d_node, nullptr, 0, int32_t(m1.list.size()), m1.h_list.dev(), m1.d_adj_off, m1.d_adj,
                width, m1.d_words + m1.next_word, m1.d_words + (m1.next_word ^ 1), seed, memo1_spread(int64_t(m1.list.size()) * width)};
    if (int code = launch_bp_memo1_patch(a, e->stream)) {
        memo0_invalidate(e);
        return fail(BN_ERR_HIP, std::string("bp_memo1_patch launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    m1.word = m1.next_word;
    m1.next_word ^= 1;
    m1.holds = true;
    e->ev_upload_pending = true;   // the launch reads the list in place
    return BN_OK;
}

// Builds the second-sweep image from the first-sweep image, which must be the pristine one (memo0_ensure, right behind its build
// launch): one launch over all nodes with the marks ignored, the contributions back to the host and ordered once.
static int memo1_build(bn_engine* e) {
    bn_engine::Memo1& m1 = e->memo1;
    const bn_engine::Memo0& m = e->memo;
    const Plan& p = e->plan;
    hipStream_t s = e->stream;
    const size_t rec_bytes = sizeof(double) * size_t(std::max<int64_t>(p.rec_total_doubles, 1));
    const size_t node_bytes = sizeof(double) * size_t(std::max<int64_t>(p.node_doubles, 1));
    if (!m1.d_rec) {
        m1.max_degree = bn_policy::memo1_adjacency(p.n, p.in_ptr, p.in_idx, m1.adj_off, m1.adj);
        HIPCHK(dev_malloc(m1.d_rec, rec_bytes));
        HIPCHK(dev_malloc(m1.d_node, node_bytes));
        HIPCHK(dev_malloc(m1.d_cv, sizeof(double) * size_t(p.n)));
        HIPCHK(dev_malloc(m1.d_words, sizeof(unsigned long long) * 4));
        HIPCHK(dev_malloc(m1.d_img, sizeof(Memo0Image) * 9));
        HIPCHK(dev_malloc(m1.d_adj_off, sizeof(int32_t) * m1.adj_off.size()));
        HIPCHK(dev_malloc(m1.d_adj, sizeof(int32_t) * std::max<size_t>(m1.adj.size(), 1)));
        Memo0Image img[9];
        for (int w0 = 0; w0 < 3; ++w0)
            for (int w1 = 0; w1 < 3; ++w1) img[3 * w0 + w1] = Memo0Image{m1.d_rec, m1.d_node, m1.d_words + w1, m.d_words + w0};
        HIPCHK(hipMemcpy(m1.d_img, img, sizeof img, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(m1.d_adj_off, m1.adj_off.data(), sizeof(int32_t) * m1.adj_off.size(), hipMemcpyHostToDevice));
        if (!m1.adj.empty()) HIPCHK(hipMemcpy(m1.d_adj, m1.adj.data(), sizeof(int32_t) * m1.adj.size(), hipMemcpyHostToDevice));
        HIPCHK(m1.h_list.alloc(size_t(p.n)));
    }
    HIPCHK(hipMemsetAsync(m1.d_rec, 0, rec_bytes, s));     // (padding and the slots of lanes without a node: never read for a result)
    HIPCHK(hipMemsetAsync(m1.d_node, 0, node_bytes, s));
    HIPCHK(hipMemsetAsync(m1.d_words, 0, sizeof(unsigned long long) * 4, s));
    Memo1Args a{buffers_of(e), m.d_rec, m.d_node, m1.d_rec, m1.d_node, m1.d_cv, p.n, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, 0ull, 0};
    if (int code = launch_bp_memo1_build(a, s))
        return fail(BN_ERR_HIP, std::string("bp_memo1_build launch failed: ") + hipGetErrorString(hipError_t(code)));
    m1.cv.assign(size_t(p.n), 0.0);
    HIPCHK(hipMemcpyAsync(m1.cv.data(), m1.d_cv, sizeof(double) * size_t(p.n), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    m1.order.resize(size_t(p.n));
    std::iota(m1.order.begin(), m1.order.end(), 0);
    std::stable_sort(m1.order.begin(), m1.order.end(), [&](int32_t x, int32_t y) { return m1.cv[size_t(x)] > m1.cv[size_t(y)]; });
    HIPCHK(hipMemcpy(m1.d_words + 2, &m1.cv[size_t(m1.order[0])], sizeof(double), hipMemcpyHostToDevice));
    m1.applied.clear();
    m1.word = 2;
    m1.next_word = 0;
    m1.built = true;
    return BN_OK;
}

// ONE launch for the evidence in force (the staging block): marks and vectors in the tile buffers as bp_evidence_kernel writes them,
// the image's slots of the set's nodes as evidence nodes, the slots of the nodes the image held as evidence nodes and the set does
// not list as ordinary ones.  Nothing to apply and nothing to restore: no launch, sweep 0's residual is the constant word.
static int memo0_patch_level0(bn_engine* e) {
    bn_engine::Memo0& m = e->memo;
    const Plan& p = e->plan;
    const int32_t ne = e->ev_ne;
    const int32_t* nodes = ne > 0 ? reinterpret_cast<const int32_t*>(e->h_ev.get()) : nullptr;
    bn_policy::memo0_stamp(nodes, ne, p.n, m.stamp, m.epoch);
    bn_policy::memo0_restore_list(m.applied, m.stamp, m.epoch, m.restore);
    m.const_residual = bn_policy::memo0_const_residual(m.order, m.cv, m.stamp, m.epoch);
    if (ne == 0 && m.restore.empty()) {
        m.applied.clear();
        m.word = 2;
        return BN_OK;
    }
    if (!m.restore.empty()) std::memcpy(m.h_restore.get(), m.restore.data(), m.restore.size() * sizeof(int32_t));
    unsigned long long seed = 0;
    std::memcpy(&seed, &m.const_residual, sizeof seed);
    Memo0Args a{buffers_of(e), ne, e->d_ev_node, e->d_ev_off, e->d_ev_val, int32_t(m.restore.size()), m.h_restore.dev(),
                m.d_rec, m.d_node, nullptr, 0, m.d_words + m.next_word, m.d_words + (m.next_word ^ 1), seed, memo0_spread(ne + int32_t(m.restore.size()))};
    if (int code = launch_bp_memo0_patch(a, e->stream)) {
        memo0_invalidate(e);
        return fail(BN_ERR_HIP, std::string("bp_memo0_patch launch failed: ") + hipGetErrorString(hipError_t(code)));
    }
    m.word = m.next_word;
    m.next_word ^= 1;
    if (ne > 0) m.applied.assign(nodes, nodes + ne);
    else m.applied.clear();
    e->ev_upload_pending = true;   // the launch reads the staging block and the restore list in place
    return BN_OK;
}

int bn_eng::memo0_patch(bn_engine* e) {
    if (int rc = memo0_patch_level0(e)) return rc;
    return memo1_patch(e);   // (queued behind: the first-sweep image and the marks are those of the new set)
}

// Builds the image where there is none (the first run that can use it; after bn_reload_cpt; after a failed launch): one launch over
// all nodes as ordinary nodes, the contributions back to the host and ordered once, then the evidence in force.
int bn_eng::memo0_ensure(bn_engine* e) {
    bn_engine::Memo0& m = e->memo;
    if (m.valid) return BN_OK;
    const Plan& p = e->plan;
    hipStream_t s = e->stream;
    const size_t rec_bytes = sizeof(double) * size_t(std::max<int64_t>(p.rec_total_doubles, 1));
    const size_t node_bytes = sizeof(double) * size_t(std::max<int64_t>(p.node_doubles, 1));
    if (!m.d_rec) {
        HIPCHK(dev_malloc(m.d_rec, rec_bytes));
        HIPCHK(dev_malloc(m.d_node, node_bytes));
        HIPCHK(dev_malloc(m.d_cv, sizeof(double) * size_t(p.n)));
        HIPCHK(dev_malloc(m.d_words, sizeof(unsigned long long) * 4));
        HIPCHK(dev_malloc(m.d_img, sizeof(Memo0Image) * 3));
        Memo0Image img[3];
        for (int w = 0; w < 3; ++w) img[w] = Memo0Image{m.d_rec, m.d_node, m.d_words + w, nullptr};
        HIPCHK(hipMemcpy(m.d_img, img, sizeof img, hipMemcpyHostToDevice));
        HIPCHK(m.h_restore.alloc(size_t(p.n)));
    }
    HIPCHK(hipMemsetAsync(m.d_rec, 0, rec_bytes, s));     // (padding and the slots of lanes without a node: never read for a result)
    HIPCHK(hipMemsetAsync(m.d_node, 0, node_bytes, s));
    HIPCHK(hipMemsetAsync(m.d_words, 0, sizeof(unsigned long long) * 4, s));
    Memo0Args a{buffers_of(e), 0, nullptr, nullptr, nullptr, 0, nullptr, m.d_rec, m.d_node, m.d_cv, p.n, nullptr, nullptr, 0ull, 0};
    if (int code = launch_bp_memo0_build(a, s))
        return fail(BN_ERR_HIP, std::string("bp_memo0_build launch failed: ") + hipGetErrorString(hipError_t(code)));
    m.cv.assign(size_t(p.n), 0.0);
    HIPCHK(hipMemcpyAsync(m.cv.data(), m.d_cv, sizeof(double) * size_t(p.n), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    e->ev_upload_pending = false;
    m.order.resize(size_t(p.n));
    std::iota(m.order.begin(), m.order.end(), 0);
    std::stable_sort(m.order.begin(), m.order.end(), [&](int32_t x, int32_t y) { return m.cv[size_t(x)] > m.cv[size_t(y)]; });
    HIPCHK(hipMemcpy(m.d_words + 2, &m.cv[size_t(m.order[0])], sizeof(double), hipMemcpyHostToDevice));
    m.applied.clear();
    m.word = 2;
    m.next_word = 0;
    m.valid = true;
    if (e->memo1.enabled != 0) {   // the second-sweep image, while the first-sweep one is still the pristine one
        if (int rc = memo1_build(e)) { memo0_invalidate(e); return rc; }
    }
    return memo0_patch(e);
}
