// bn_kernels.hip -- hand-written gfx950 kernels for synchronous (Jacobi) loopy belief propagation,
// one launch per sweep.
//
// One launch = one iteration of the reference's while(true) loop
// (bayesian/inference/belief_propagation.hpp:75-148): message phase (:78-88), node phase
// (:91-101), residual (:105-131) and commit (:135-143, here a buffer swap) are fused into a
// single pass in which every node's CPT is read exactly once.  Work decomposition: one 64-lane
// wavefront per tile (bn_plan.hpp); the tile code is in bn_tiles.hpp.
//
// Iteration 0 reads nothing but the CPT and the evidence: the reference's initial state (:33-73)
// is all-ones messages, pi = lambda = 1 (roots: their CPT row), so it is synthesised in registers
// instead of being written to HBM by an initialisation pass and read back.
//
// Convergence is decided on the device: sweep s accumulates max|new-old| over messages into a
// ring of 256 slots (atomic umax on the bit pattern of a non-negative double); ONE extra wave of
// launch s+1 reduces them and marks the run done once maximum_difference < eps (:147); every later
// launch returns at once, so the host enqueues launches ahead without synchronising per sweep.
#include "bn_sweep.hpp"

namespace bnmi {

// The same iteration for networks WITHOUT register-resident tiles (any-arity and one-lane tiles
// only): those tiles need a third of the registers and are latency-bound, so this instantiation
// runs at twice the occupancy (4 waves per SIMD).
template <bool BATCH>
__global__ __launch_bounds__(kBlockThreads, 4) void bp_sweep_light_kernel(SweepArgs a_in) {
    const SweepArgs a = BATCH ? sweep_args_of_set(a_in) : a_in;
    __shared__ double flat_lds[kWavesPerBlock][kFlatLds];
    const BpBuffers& b = a.b;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int done = __hip_atomic_load(&b.ctl->done_run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.run_id;
    const int tile = a.tile_begin + logical_block() * kWavesPerBlock + wave;
    if (tile >= a.tile_end) {
        if (done == 0 && a.book != 0 && tile == a.tile_end) sweep_bookkeeping(a, lane);
        return;
    }
    const IO io{a.rec_in, a.rec_out, a.node_in, a.node_out, a.sweep == 0};
#ifdef BN_TILE_CLOCK
    const unsigned long long t_entry = wall_clock64();
#endif
    const TileDesc td = b.tiles[tile];
    if (done != 0) return;
    const double wres = run_tile_light(b, io, td, lane, flat_lds[wave]);
    publish_residual(b, a.rec_out, tile, wres, lane);
#ifdef BN_TILE_CLOCK
    if (lane == 0 && td.slot_base < kTileClockTiles) {
        g_tile_clock[td.slot_base][9] = t_entry;
        g_tile_clock[td.slot_base][11] = wall_clock64();
    }
#endif
}

// bn_bp_set_evidence: apply the evidence (belief_propagation.hpp:68-73) to the nodes this rank owns:
// pi(v) = lambda(v) = the given vector in the buffer iteration 0 reads, node marked
// (preconditional_node_: the slot takes the mark value of this evidence set, so the previous set's marks need no
// clearing).  The arrays are read straight from the caller-side staging block in page-locked host memory.  The marks and vectors stay
// until the next bn_bp_set_evidence: a marked node's vectors are copied forward by every sweep, so
// both buffers keep holding them and any number of runs can follow without touching them again.
__global__ __launch_bounds__(kBlockThreads) void bp_evidence_kernel(EvidenceArgs a) {
    const BpBuffers& b = a.b;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.ne) return;
    const int v = a.ev_node[j];
    const int t = b.node_tile[v];
    if (t < 0) return;  // owned by another rank
    const TileDesc td = b.tiles[t];
    const int nl = b.node_nl[v];
    const int half = ((td.kv + 1) & ~1) >> 1;
    for (int i = 0; i < td.kv; ++i) {
        const double x = a.ev_val[a.ev_off[j] + i];
        b.node0[td.node_base + vidx(0, i, td.npt, nl)] = x;
        b.node0[td.node_base + vidx(half, i, td.npt, nl)] = x;
        b.node1[td.node_base + vidx(0, i, td.npt, nl)] = x;
        b.node1[td.node_base + vidx(half, i, td.npt, nl)] = x;
    }
    b.frozen[td.slot_base + nl] = b.frozen_mark;
}

// ---- the first-sweep image of the resident path (bn_device.hpp Memo0Args) ----------------------------------------------------
// Sweep 0 of a run reads no message (every message, pi(v) of a node with parents and lambda(v) start at 1.0, a root's pi(v) at its
// CPT row, an evidence node's two vectors at its evidence), so what a node's lane leaves behind -- its pi-messages to its children,
// its lambda-messages to its parents, its new pi(v) / lambda(v), its share of the residual -- is a function of its own CPT and its own
// evidence alone.  memo0_node computes exactly that for ONE node and writes it into the image: the slots this node's lane writes in
// sweep 0 of bn_resident.hip's resident_tile, nothing else.  `frozen`: the node carries the evidence vector `ev`.  Every sum and
// product keeps resident_tile's association and order of terms for first == true (multiplications by the synthesised 1.0 are exact
// and left out; roots keep 0.0 + cpt; normalisation is unguarded), so the image holds the very bits sweep 0 would have written.
// Covers what the barrier form of the resident kernel admits: one lane per node, uniform arity 2..4, at most two parents, at most 8
// children.  Returns the node's residual contribution: max |new - 1.0| over its outgoing messages, NaN terms dropped (res_acc).
// One instantiation per shape (K, M): the patch launch stands in front of every query that changes the evidence, and with run-time
// loops a lane's 64 table reads followed each other one memory latency apart (~60 us per launch on the 316 x 316 grid); unrolled,
// the table and the references are requested together and waited for once.
template <int K, int M>
__device__ __forceinline__ double memo0_node_t(const BpBuffers& b, const TileDesc& td, int nl, bool frozen, const double (&ev)[4], double* rec,
                                               double* node) {
    constexpr int KP = (K + 1) & ~1, H = KP / 2, C = ipow(K, M), S = K * C, SP = (S + 1) & ~1;
    const double2_t* cp = reinterpret_cast<const double2_t*>(b.cpt + td.cpt_base) + nl;  // entry e of the i-major image: chunk e / 2 (bn_plan.hpp)
    double cpt[SP];
#pragma unroll
    for (int q = 0; q < SP / 2; ++q) {
        const double2_t x = cp[q * kWave];
        cpt[2 * q] = x.x;
        cpt[2 * q + 1] = x.y;
    }
    const MsgRef* orf = b.out_refs + td.out_base + nl;
    MsgRef oref[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        oref[c] = MsgRef{-1, 0};
        if (c < td.cmax) oref[c] = orf[c * kWave];
    }
    auto put = [&](double* base, int64_t at2, const double (&x)[K], int h) {  // chunk h of a vector as one double2, padding zero
        double2_t y;
        y.x = x[2 * h];
        y.y = (2 * h + 1 < K) ? x[(2 * h + 1 < K) ? 2 * h + 1 : 0] : 0.0;
        reinterpret_cast<double2_t*>(base)[at2] = y;
    };
    double piv[K], lav[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        piv[i] = frozen ? ev[i] : (M == 0 ? cpt[i] : 1.0);
        lav[i] = frozen ? ev[i] : 1.0;
    }
    double res = 0.0;
    // parent role: lambda(v) = the product of the children's lambda-messages (all 1.0), normalised; the pi-message to each child =
    // pi(v) times the other children's lambda-messages (1.0), normalised: the same vector for every child
    double lan[K], u[K];
#pragma unroll
    for (int i = 0; i < K; ++i) { lan[i] = 1.0; u[i] = piv[i]; }
    normalize_k<K>(lan);
    normalize_k<K>(u);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const Loc l = decode_ref(oref[c], H);
        if (l.has) {
#pragma unroll
            for (int i = 0; i < K; ++i) res = res_acc(res, fabs(u[i] - 1.0));
#pragma unroll
            for (int h = 0; h < H; ++h) put(rec, l.pi + int64_t(h) * l.stride, u, h);
        }
    }
    // child role: pi(v)[ib] = the sum of the own state's CPT entries in assignment order (the parents' pi-messages are 1.0);
    // lambda-message to parent j, entry u = sum over own states (outer) and the other parent's states (inner) of lambda(v)[ib] * cpt
    double pin[K], out[M > 0 ? M : 1][K];
#pragma unroll
    for (int j = 0; j < (M > 0 ? M : 1); ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) out[j][i] = 0.0;
#pragma unroll
    for (int ib = 0; ib < K; ++ib) {
        if constexpr (M == 0) {
            pin[ib] = 0.0 + cpt[ib];
        } else {
            double acc = 0.0;
            if constexpr (M == 2) {
#pragma unroll
                for (int u0 = 0; u0 < K; ++u0)
#pragma unroll
                    for (int u1 = 0; u1 < K; ++u1) {
                        const double r = cpt[ib * C + u0 * K + u1];
                        acc += r;
                        const double tt = lav[ib] * r;
                        out[0][u0] += tt;
                        out[1][u1] += tt;
                    }
            } else {
#pragma unroll
                for (int x = 0; x < K; ++x) acc += cpt[ib * C + x];
#pragma unroll
                for (int x = 0; x < K; ++x) out[0][x] += lav[ib] * cpt[ib * C + x];
            }
            pin[ib] = acc;
        }
    }
    normalize_k<K>(pin);
    const int64_t rbase = td.rec_base / 2 + nl;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        normalize_k<K>(out[j]);
#pragma unroll
        for (int i = 0; i < K; ++i) res = res_acc(res, fabs(out[j][i] - 1.0));
#pragma unroll
        for (int h = 0; h < H; ++h) put(rec, rbase + int64_t((j * 2 + 1) * H + h) * kWave, out[j], h);
    }
    // the node's new vectors; an evidence node keeps its evidence
    if (!frozen) {
#pragma unroll
        for (int i = 0; i < K; ++i) { piv[i] = pin[i]; lav[i] = lan[i]; }
    }
    const int64_t nbase = td.node_base / 2 + nl;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        put(node, nbase + int64_t(h) * kWave, piv, h);
        put(node, nbase + int64_t(H + h) * kWave, lav, h);
    }
    return res;
}

__device__ __forceinline__ double memo0_node(const BpBuffers& b, int v, bool frozen, const double (&ev)[4], double* rec, double* node) {
    const int t = b.node_tile[v];
    if (t < 0) return 0.0;
    const TileDesc td = b.tiles[t];
    if (td.variant != kVariantUniform || td.npt != kWave || td.cmax > 8) return 0.0;  // (the host builds no image for such a plan)
    const int nl = b.node_nl[v];
    switch (td.kv * 4 + td.m) {
        case 2 * 4 + 0: return memo0_node_t<2, 0>(b, td, nl, frozen, ev, rec, node);
        case 2 * 4 + 1: return memo0_node_t<2, 1>(b, td, nl, frozen, ev, rec, node);
        case 2 * 4 + 2: return memo0_node_t<2, 2>(b, td, nl, frozen, ev, rec, node);
        case 3 * 4 + 0: return memo0_node_t<3, 0>(b, td, nl, frozen, ev, rec, node);
        case 3 * 4 + 1: return memo0_node_t<3, 1>(b, td, nl, frozen, ev, rec, node);
        case 3 * 4 + 2: return memo0_node_t<3, 2>(b, td, nl, frozen, ev, rec, node);
        case 4 * 4 + 0: return memo0_node_t<4, 0>(b, td, nl, frozen, ev, rec, node);
        case 4 * 4 + 1: return memo0_node_t<4, 1>(b, td, nl, frozen, ev, rec, node);
        case 4 * 4 + 2: return memo0_node_t<4, 2>(b, td, nl, frozen, ev, rec, node);
        default: return 0.0;
    }
}

// the image of the network without evidence, and every node's own residual contribution
__global__ __launch_bounds__(kBlockThreads) void bp_memo0_build_kernel(Memo0Args a) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n) return;
    const double none[4] = {0.0, 0.0, 0.0, 0.0};
    a.cv[v] = memo0_node(a.b, v, false, none, a.rec, a.node);
}

// One launch per evidence set: what bp_evidence_kernel does (marks, vectors in both node buffers) for the nodes of the new set, their
// slots of the image recomputed as evidence nodes, and the slots of the nodes that lose their evidence recomputed as ordinary nodes.
// The evidence nodes' residual contributions and the seed go into *word (bit patterns of non-negative doubles order like unsigned
// integers), which the previous patch launch left zero; this one leaves the next launch's word zero.
__global__ __launch_bounds__(kWave) void bp_memo0_patch_kernel(Memo0Args a) {
    const BpBuffers& b = a.b;
    // one node per 2^spread lanes: a node's table is 32 scattered lines, and a wave of 64 such nodes keeps one CU's address path busy
    // for microseconds -- spread out, the launch's few thousand nodes use the whole chip
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (g & ((1 << a.spread) - 1)) == 0 ? (g >> a.spread) : 0x7fffffff;
    // The lists are read in place from page-locked host memory: a read is a trip over the bus.  Everything that depends on j alone is
    // requested at once (node, offset, length), then the values and -- beside them, in device memory -- the node's tile, its CPT and
    // its references: two trips over the bus on the lane's critical path, as in bp_evidence_kernel, with the device reads under the second.
    const bool frozen = j < a.ne, restore = !frozen && j < a.ne + a.n_restore;
    int v = -1, off = 0, len = 0;
    if (frozen) {
        v = a.ev_node[j];
        off = a.ev_off[j];
        len = a.ev_off[j + 1] - off;
    } else if (restore) {
        v = a.restore[j - a.ne];
    }
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    if (frozen) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < len) x[i] = a.ev_val[off + i];
    }
    unsigned long long bits = a.seed;
    const int t = v >= 0 ? b.node_tile[v] : -1;
    if (t >= 0) {  // (else: no node for this lane, or one owned by another rank)
        if (frozen) {
            const TileDesc td = b.tiles[t];
            const int nl = b.node_nl[v];
            const int half = ((td.kv + 1) & ~1) >> 1;
            for (int i = 0; i < td.kv; ++i) {
                const double y = i < 4 ? x[i & 3] : a.ev_val[off + i];
                b.node0[td.node_base + vidx(0, i, td.npt, nl)] = y;
                b.node0[td.node_base + vidx(half, i, td.npt, nl)] = y;
                b.node1[td.node_base + vidx(0, i, td.npt, nl)] = y;
                b.node1[td.node_base + vidx(half, i, td.npt, nl)] = y;
            }
            b.frozen[td.slot_base + nl] = b.frozen_mark;
        }
        const unsigned long long p = (unsigned long long)__double_as_longlong(memo0_node(b, v, frozen, x, a.rec, a.node));
        if (frozen) bits = p > bits ? p : bits;
    }
    bits = wave_umax(bits);
    if ((threadIdx.x & (kWave - 1)) == 0) __hip_atomic_fetch_max(a.word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j == 0) *a.word_next = 0ull;
}

// ---- the second-sweep image of the resident path (bn_device.hpp Memo1Args) ---------------------------------------------------
// One Jacobi sweep with first == false for ONE node, from a source image (records + node vectors) into a destination image of the
// same layout: it reads the node's CPT, its vectors, its children's lambda-messages, its parents' pi-messages and its own previous
// outgoing messages from the source and writes exactly the slots this node's lane writes in a sweep of bn_resident.hip's
// resident_tile -- its pi-messages into the children's in-edge slots (out_refs), its lambda-messages into its own in-edge slots, its
// new pi(v) / lambda(v) -- into the destination.  `frozen`: the node carries evidence, its vectors in the source are that evidence
// and stay.  Level-agnostic: the source may be any sweep's state, so a later change can chain it.  Every sum and product keeps
// resident_tile's association and order of terms (bn_tiles.hpp tile_uniform is the statement-for-statement source): lambda(v) is
// the product of the children's lambda-messages in ascending child order from 1.0, the pi-message to child c is pi(v) times the OTHER
// children's lambda-messages in ascending order, a missing child contributes an exact 1.0; pi(v)[i] sums (cpt pi0) pi1 over the
// assignments in ascending order, the lambda-message to parent j sums (lambda(v)[i] cpt) pi_other with the own state outer;
// normalisation is unguarded and res_acc drops NaN terms.  Covers what memo0_node covers.  Returns the node's residual contribution.
// One instantiation per shape (K, M), as memo0_node_t and for its reasons: everything is requested at once and waited for once.
template <int K, int M>
__device__ __forceinline__ double memo_step_node_t(const BpBuffers& b, const TileDesc& td, int nl, bool frozen, const double* src_rec,
                                                   const double* src_node, double* rec, double* node) {
    constexpr int KP = (K + 1) & ~1, H = KP / 2, C = ipow(K, M), S = K * C, SP = (S + 1) & ~1;
    const double2_t* cp = reinterpret_cast<const double2_t*>(b.cpt + td.cpt_base) + nl;
    double cpt[SP];
#pragma unroll
    for (int q = 0; q < SP / 2; ++q) {
        const double2_t x = cp[q * kWave];
        cpt[2 * q] = x.x;
        cpt[2 * q + 1] = x.y;
    }
    const MsgRef* orf = b.out_refs + td.out_base + nl;
    Loc ol[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        MsgRef r{-1, 0};
        if (c < td.cmax) r = orf[c * kWave];
        ol[c] = decode_ref(r, H);
    }
    const double2_t* sr = reinterpret_cast<const double2_t*>(src_rec);
    const int64_t rbase = td.rec_base / 2 + nl;  // this node's slot in its tile's record block (double2 units)
    auto in_idx = [&](int j, int part, int h) -> int64_t { return rbase + int64_t((j * 2 + part) * H + h) * kWave; };
    auto put = [&](double* base, int64_t at2, const double (&x)[K], int h) {  // chunk h of a vector as one double2, padding zero
        double2_t y;
        y.x = x[2 * h];
        y.y = (2 * h + 1 < K) ? x[(2 * h + 1 < K) ? 2 * h + 1 : 0] : 0.0;
        reinterpret_cast<double2_t*>(base)[at2] = y;
    };
    // the node's vectors, the parents' pi-messages, this node's previous lambda-messages
    const double2_t* nin = reinterpret_cast<const double2_t*>(src_node) + td.node_base / 2 + nl;
    double piv[KP], lav[KP];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        const double2_t x = nin[h * kWave], y = nin[(H + h) * kWave];
        piv[2 * h] = x.x; piv[2 * h + 1] = x.y;
        lav[2 * h] = y.x; lav[2 * h + 1] = y.y;
    }
    double pim[M > 0 ? M : 1][KP], oldl[M > 0 ? M : 1][KP];
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const double2_t x = sr[in_idx(j, 0, h)], y = sr[in_idx(j, 1, h)];
            pim[j][2 * h] = x.x; pim[j][2 * h + 1] = x.y;
            oldl[j][2 * h] = y.x; oldl[j][2 * h + 1] = y.y;
        }
    // the children's lambda-messages and this node's previous pi-messages (a missing child reads record 0 and counts as 1.0)
    double lkc[8][KP], oldp[8][KP];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int i = 0; i < KP; ++i) { lkc[c][i] = 1.0; oldp[c][i] = 1.0; }
        if (c < td.cmax) {
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const double2_t y = sr[ol[c].lam + h * ol[c].stride], x = sr[ol[c].pi + h * ol[c].stride];
                lkc[c][2 * h] = ol[c].has ? y.x : 1.0;
                lkc[c][2 * h + 1] = ol[c].has ? y.y : 1.0;
                oldp[c][2 * h] = x.x; oldp[c][2 * h + 1] = x.y;
            }
        }
    }
    double res = 0.0;
    // ---- parent role: lambda(v), the pi-message to every child
    double lan[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double acc = 1.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc *= lkc[c][i];
        lan[i] = acc;
    }
    normalize_k<K>(lan);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c < td.cmax) {
            double u[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                double acc = piv[i];
#pragma unroll
                for (int x = 0; x < 8; ++x)
                    if (x != c) acc *= lkc[x][i];
                u[i] = acc;
            }
            normalize_k<K>(u);
            if (ol[c].has) {
#pragma unroll
                for (int i = 0; i < K; ++i) res = res_acc(res, fabs(u[i] - oldp[c][i]));
#pragma unroll
                for (int h = 0; h < H; ++h) put(rec, ol[c].pi + int64_t(h) * ol[c].stride, u, h);
            }
        }
    }
    // ---- child role: pi(v) and the lambda-message to every parent
    double pin[K], out[M > 0 ? M : 1][K];
#pragma unroll
    for (int j = 0; j < (M > 0 ? M : 1); ++j)
#pragma unroll
        for (int i = 0; i < K; ++i) out[j][i] = 0.0;
#pragma unroll
    for (int ib = 0; ib < K; ++ib) {
        if constexpr (M == 0) {
            pin[ib] = 0.0 + cpt[ib];
        } else {
            double acc = 0.0;
            if constexpr (M == 2) {
#pragma unroll
                for (int rr = 0; rr < K; ++rr)
#pragma unroll
                    for (int x = 0; x < K; ++x) {
                        const double r = cpt[ib * C + rr * K + x];
                        double value = r * pim[0][rr];
                        value *= pim[1][x];
                        acc += value;
                        const double t = lav[ib] * r;
                        out[0][rr] += t * pim[1][x];
                        out[1][x] += t * pim[0][rr];
                    }
            } else {
#pragma unroll
                for (int x = 0; x < K; ++x) {
                    double value = cpt[ib * C + x];
                    value *= pim[0][x];
                    acc += value;
                }
#pragma unroll
                for (int x = 0; x < K; ++x) out[0][x] += lav[ib] * cpt[ib * C + x];
            }
            pin[ib] = acc;
        }
    }
    normalize_k<K>(pin);
#pragma unroll
    for (int j = 0; j < M; ++j) {
        normalize_k<K>(out[j]);
#pragma unroll
        for (int i = 0; i < K; ++i) res = res_acc(res, fabs(out[j][i] - oldl[j][i]));
#pragma unroll
        for (int h = 0; h < H; ++h) put(rec, in_idx(j, 1, h), out[j], h);
    }
    // the node's new vectors; an evidence node keeps its evidence
    double po[K], lo[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        po[i] = frozen ? piv[i] : pin[i];
        lo[i] = frozen ? lav[i] : lan[i];
    }
    const int64_t nbase = td.node_base / 2 + nl;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        put(node, nbase + int64_t(h) * kWave, po, h);
        put(node, nbase + int64_t(H + h) * kWave, lo, h);
    }
    return res;
}

__device__ __forceinline__ double memo_step_node(const BpBuffers& b, int v, bool ignore_marks, const double* src_rec, const double* src_node,
                                                 double* rec, double* node) {
    const int t = b.node_tile[v];
    if (t < 0) return 0.0;
    const TileDesc td = b.tiles[t];
    if (td.variant != kVariantUniform || td.npt != kWave || td.cmax > 8) return 0.0;  // (the host builds no image for such a plan)
    const int nl = b.node_nl[v];
    const bool frozen = !ignore_marks && b.frozen[td.slot_base + nl] == b.frozen_mark;
    switch (td.kv * 4 + td.m) {
        case 2 * 4 + 0: return memo_step_node_t<2, 0>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 2 * 4 + 1: return memo_step_node_t<2, 1>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 2 * 4 + 2: return memo_step_node_t<2, 2>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 3 * 4 + 0: return memo_step_node_t<3, 0>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 3 * 4 + 1: return memo_step_node_t<3, 1>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 3 * 4 + 2: return memo_step_node_t<3, 2>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 4 * 4 + 0: return memo_step_node_t<4, 0>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 4 * 4 + 1: return memo_step_node_t<4, 1>(b, td, nl, frozen, src_rec, src_node, rec, node);
        case 4 * 4 + 2: return memo_step_node_t<4, 2>(b, td, nl, frozen, src_rec, src_node, rec, node);
        default: return 0.0;
    }
}

// the second-sweep image of the network without evidence (the source is the pristine first-sweep image; the marks of whatever set
// is in force are ignored), and every node's own residual contribution in sweep 1
__global__ __launch_bounds__(kWave) void bp_memo1_build_kernel(Memo1Args a) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n) return;
    a.cv[v] = memo_step_node(a.b, v, true, a.src_rec, a.src_node, a.rec, a.node);
}

// One launch per evidence set, behind the first-sweep patch on the same stream: thread (j, q) recomputes slot q of the closed
// neighbourhood of listed node j -- q = 0 the node itself, then its parents and children (node-level CSR in device memory).  The marks
// and the first-sweep image are those of the new set.  *word receives max(seed, every contribution computed): a recomputed node
// outside N[E] gives its pristine contribution again, which the seed bounds.
__global__ __launch_bounds__(kWave) void bp_memo1_patch_kernel(Memo1Args a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int item = (g & ((1 << a.spread) - 1)) == 0 ? (g >> a.spread) : 0x7fffffff;
    const int j = item / a.width, q = item - j * a.width;
    int v = -1;
    if (j < a.n_list) {
        const int v0 = a.list[j];  // (page-locked host memory: one trip over the bus; the rest is device memory)
        if (q == 0) {
            v = v0;
        } else {
            const int o = a.adj_off[v0] + q - 1;
            if (o < a.adj_off[v0 + 1]) v = a.adj[o];
        }
    }
    unsigned long long bits = a.seed;
    if (v >= 0) {
        const unsigned long long p = (unsigned long long)__double_as_longlong(memo_step_node(a.b, v, false, a.src_rec, a.src_node, a.rec, a.node));
        bits = p > bits ? p : bits;
    }
    bits = wave_umax(bits);
    if ((threadIdx.x & (kWave - 1)) == 0) __hip_atomic_fetch_max(a.word, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (g == 0) *a.word_next = 0ull;
}

// This rank's residual slots in both buffers. A finished run leaves them zero itself
// (bp_finish_kernel); this kernel runs only after a run that did not end normally.
__global__ __launch_bounds__(kBlockThreads) void bp_reset_kernel(BpBuffers b) {
    unsigned long long* r0 = res_row(b, b.rec0, b.rank);
    unsigned long long* r1 = res_row(b, b.rec1, b.rank);
    for (int q = threadIdx.x; q < kResSlots; q += kBlockThreads) { r0[q] = 0ull; r1[q] = 0ull; }
}

// After a batch of sweeps (and their exchanges).  Wave 0 of block 0 settles the run: if no sweep
// launch marked it done, it reduces the last launched sweep's residual and decides (converged /
// max_sweeps reached / go on), reports to the pinned host block, and -- once the run is over -- leaves
// the residual slots zero for the next run.  Every other wave writes belief = normalize(pi % lambda)
// (:151-158) for its tile's nodes from the buffer the last executed sweep wrote; when the host has to
// go on (predicted sweep count too low) those beliefs are simply overwritten by the next finish.
__global__ __launch_bounds__(kBlockThreads) void bp_finish_kernel(FinishArgs a) {
    BpBuffers b = a.b;
    Ctl* host_ctl = a.host_ctl;
    if (gridDim.y > 1) {  // batched run: one evidence set per y
        shift_to_set(b, a.sets, blockIdx.y);
        host_ctl += blockIdx.y;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    // Marked by a sweep launch = a previous kernel, or by wave 0 of this one (below, which releases the fields it wrote
    // before the mark).  The mark and then, behind it, the sweep count are read with L1-bypassing loads: what the
    // release made visible in L2 is what they see.  (An ACQUIRE load here invalidated the CU's L1 once per wave --
    // 65 536 times on the 2048x2048 grid -- and held this kernel at ~0.8 TB/s: 595 us there, 17 us on the 316x316 grid.)
    const bool marked = __hip_atomic_load(&b.ctl->done_run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.run_id;
    int n_sweeps = a.sweeps_launched;
    if (marked) n_sweeps = __hip_atomic_load(&b.ctl->n_sweeps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0 && wave == 0) {
        int done = 1;
        double r = marked ? __hip_atomic_load(&b.ctl->last_res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        unsigned long long t_last = marked ? __hip_atomic_load(&b.ctl->t_last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : wall_clock64();
        if (marked && !(r < a.eps)) done = 2;  // marked by an earlier finish of this run that stopped it at max_sweeps
        if (!marked) {  // sweep (launched-1) wrote buffer (launched & 1)
            r = reduce_residual(b, (a.sweeps_launched & 1) ? b.rec1 : b.rec0, lane);
            if (lane == 0 && a.sweeps_launched - 1 < b.res_cap) b.res_hist[a.sweeps_launched - 1] = r;
            done = (r < a.eps) ? 1 : (a.final_batch ? 2 : 0);
        }
        if (lane == 0) {
            host_ctl->last_res = r; host_ctl->n_sweeps = n_sweeps;
            host_ctl->t_first = b.ctl->t_first; host_ctl->t_last = t_last;
            host_ctl->run_id = a.run_id; host_ctl->done = done;
            if (!marked && done != 0) {
                // the run ends here: mark it on the device too, so that launches a batched run still issues for
                // its other evidence sets leave this one alone
                b.ctl->n_sweeps = n_sweeps; b.ctl->last_res = r; b.ctl->t_last = t_last;
                __hip_atomic_store(&b.ctl->done_run, a.run_id, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (done != 0) {
            unsigned long long* r0 = res_row(b, b.rec0, b.rank);
            unsigned long long* r1 = res_row(b, b.rec1, b.rank);
#pragma unroll
            for (int q = 0; q < kResSlots / kWave; ++q) { r0[q * kWave + lane] = 0ull; r1[q * kWave + lane] = 0ull; }
        }
    }
    const int tile = blockIdx.x * kWavesPerBlock + wave;
    if (tile >= b.n_tiles) return;
    tile_beliefs(b, b.tiles[tile], (n_sweeps & 1) ? b.node1 : b.node0, lane);
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static inline int hip_rc(hipError_t e) { return e == hipSuccess ? 0 : int(e); }

int launch_bp_evidence(const EvidenceArgs& a, void* stream) {
    if (a.ne <= 0) return 0;
    const int blocks = (a.ne + kBlockThreads - 1) / kBlockThreads;
    (void)hipGetLastError();  // drop any stale error of this thread
    hipLaunchKernelGGL(bp_evidence_kernel, dim3(blocks), dim3(kBlockThreads), 0, (hipStream_t)stream, a);
    return hip_rc(hipGetLastError());
}
int launch_bp_memo0_build(const Memo0Args& a, void* stream) {
    if (a.n <= 0) return 0;
    const int blocks = (a.n + kBlockThreads - 1) / kBlockThreads;
    (void)hipGetLastError();  // drop any stale error of this thread
    hipLaunchKernelGGL(bp_memo0_build_kernel, dim3(blocks), dim3(kBlockThreads), 0, (hipStream_t)stream, a);
    return hip_rc(hipGetLastError());
}
int launch_bp_memo0_patch(const Memo0Args& a, void* stream) {
    const int64_t work = int64_t(a.ne + a.n_restore) << a.spread;   // (0: one block still seeds the word)
    const int blocks = work > 0 ? int((work + kWave - 1) / kWave) : 1;
    (void)hipGetLastError();  // drop any stale error of this thread
    hipLaunchKernelGGL(bp_memo0_patch_kernel, dim3(blocks), dim3(kWave), 0, (hipStream_t)stream, a);
    return hip_rc(hipGetLastError());
}
int launch_bp_memo1_build(const Memo1Args& a, void* stream) {
    if (a.n <= 0) return 0;
    const int blocks = (a.n + kWave - 1) / kWave;
    (void)hipGetLastError();  // drop any stale error of this thread
    hipLaunchKernelGGL(bp_memo1_build_kernel, dim3(blocks), dim3(kWave), 0, (hipStream_t)stream, a);
    return hip_rc(hipGetLastError());
}
int launch_bp_memo1_patch(const Memo1Args& a, void* stream) {
    const int64_t work = (int64_t(a.n_list) * a.width) << a.spread;   // (0: one block still seeds the word)
    if (a.width <= 0 || work > 0x7fffffff) return int(hipErrorInvalidValue);  // (the host's work limit keeps a launch far below)
    const int blocks = work > 0 ? int((work + kWave - 1) / kWave) : 1;
    (void)hipGetLastError();  // drop any stale error of this thread
    hipLaunchKernelGGL(bp_memo1_patch_kernel, dim3(blocks), dim3(kWave), 0, (hipStream_t)stream, a);
    return hip_rc(hipGetLastError());
}
int launch_bp_reset(const BpBuffers& b, void* stream) {
    (void)hipGetLastError();  // drop any stale error of this thread
    hipLaunchKernelGGL(bp_reset_kernel, dim3(1), dim3(kBlockThreads), 0, (hipStream_t)stream, b);
    return hip_rc(hipGetLastError());
}
// variants: bit v set = the plan has tiles of variant v (bn_plan.hpp); light: any-arity / one-lane tiles only
int launch_bp_sweep(const SweepArgs& a, int grid_blocks, int n_sets, bool nontemporal, bool light, int variants, void* stream) {
    (void)hipGetLastError();  // drop any stale error of this thread
    if (light) {
        if (n_sets > 1)
            hipLaunchKernelGGL(bp_sweep_light_kernel<true>, dim3(grid_blocks, n_sets), dim3(kBlockThreads), 0, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL(bp_sweep_light_kernel<false>, dim3(grid_blocks), dim3(kBlockThreads), 0, (hipStream_t)stream, a);
        return hip_rc(hipGetLastError());
    }
    if (variants & ((1 << kVariantFlat) | (1 << kVariantGeneric))) return launch_bp_sweep_all(a, grid_blocks, n_sets, stream);
    if (variants & (1 << kVariantGroup)) return launch_bp_sweep_ug(a, grid_blocks, n_sets, nontemporal, stream);
    return launch_bp_sweep_u(a, grid_blocks, n_sets, nontemporal, stream);
}
int launch_bp_finish(const FinishArgs& a, int grid_blocks, int n_sets, void* stream) {
    (void)hipGetLastError();  // drop any stale error of this thread
    hipLaunchKernelGGL(bp_finish_kernel, dim3(grid_blocks, n_sets > 1 ? n_sets : 1), dim3(kBlockThreads), 0, (hipStream_t)stream, a);
    return hip_rc(hipGetLastError());
}

}  // namespace bnmi

BN_TILE_CLOCK_GETTER(bn_debug_tile_clock_light)
