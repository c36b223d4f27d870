// bn_jt.hip -- junction-tree propagation on gfx950: the base potentials, and the two-pass run of one evidence set per workgroup,
// as a sum run (jt_kernel: marginals), as a max run (jt_mpe_kernel: exact MPE) and as the E-step of exact expectation-maximisation
// (jt_em_kernel: the sum run of a pattern row and its family posteriors, with the small kernel of its sums; the M-step is bn_em.hip's)
// (rules: bn_jt.hpp; item tables: bn_jt_plan.hpp).  Every phase is written once: the potentials over a source of the home nodes'
// factors, the walk (collect and distribute) over an operation -- JtSum or JtMax, the decode riding the max walk as hooks that the
// sum walk does not have -- and the read-out over the same operation; the three kernels are entry points that put them together.
// The same item code runs over LDS (form 1) and over the set's slice of device scratch (form 2): the kernels are templates over
// where the state lives, so the compiler sees the address space.  A workgroup reads and writes its own state only; every phase
// ends in __syncthreads(), and no lane waits on anything else.
#include <hip/hip_runtime.h>

#include "bn_jt.hpp"
#include "bn_launch.hpp"

namespace bnmi {
namespace {

constexpr int kJtLdsThreads = 256;    // form 1
constexpr int kJtMemThreads = 1024;   // form 2

// psi0[g] = 1.0 x the entries of the clique's CPTs at entry g's assignment, ascending node id
__global__ void __launch_bounds__(256) jt_base_kernel(JtBaseArgs a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.pot_cells) return;
    const int c = a.ent_clique[g];
    const int e = g - a.cliques[c].pot_off;
    double v = 1.0;
    for (int t = a.asg_ptr[c]; t < a.asg_ptr[c + 1]; ++t) {
        const JtAsg s = a.asg[t];
        int64_t at = s.cpt_off;
        for (int f = s.fam_lo; f < s.fam_hi; ++f) {
            const JtFam m = a.fam[f];
            at += int64_t((e / m.stride) % m.k) * m.cstride;
        }
        v *= a.cpt[at];
    }
    a.psi0[g] = v;
}

// ---- the folds of bn_jt.hpp over the terms term(0), term(1), ... term(cnt - 1)

// two-level sum: runs of kJtRun terms added left to right from +0.0, then the run sums left to right from +0.0.  The order is the rule.
template <class F>
__device__ __forceinline__ double two_level_sum(int cnt, F term) {
    double total = 0.0;
    for (int r = 0; r < cnt; r += kJtRun) {
        const int hi = r + kJtRun < cnt ? r + kJtRun : cnt;
        double run = 0.0;
        for (int t = r; t < hi; ++t) run += term(t);
        total += run;
    }
    return total;
}

template <class F>
__device__ __forceinline__ double max_fold(int cnt, F term) {
    double acc = 0.0;
    for (int t = 0; t < cnt; ++t) {
        const double x = term(t);
        acc = acc < x ? x : acc;
    }
    return acc;
}

// the terms tab[res[0]], tab[res[1]], ...
__device__ __forceinline__ auto gathered(const double* tab, const int32_t* res) {
    return [=](int t) { return tab[res[t]]; };
}

__device__ __forceinline__ double sum_two_level(const double* tab, const int32_t* res, int cnt) { return two_level_sum(cnt, gathered(tab, res)); }

// the two operations of a run.  fold: of a clique's matching entries, onto a separator entry or a node's state; scale: of a
// separator's entries.  kDecode: the walk makes the picks of the backtrack and writes the states.
struct JtSum {
    static constexpr bool kDecode = false;
    template <class F>
    static __device__ __forceinline__ double fold(int cnt, F term) { return two_level_sum(cnt, term); }
    template <class F>
    static __device__ __forceinline__ double scale(int cnt, F term) {   // left to right from +0.0
        double s = 0.0;
        for (int j = 0; j < cnt; ++j) s += term(j);
        return s;
    }
};
struct JtMax {
    static constexpr bool kDecode = true;
    template <class F>
    static __device__ __forceinline__ double fold(int cnt, F term) { return max_fold(cnt, term); }
    template <class F>
    static __device__ __forceinline__ double scale(int cnt, F term) { return max_fold(cnt, term); }
};

// the decode's pick among the entries tab[index(0)], tab[index(1)], ... in ascending entry index: the lowest index of the largest
template <class F>
__device__ __forceinline__ int first_largest(const double* tab, int cnt, F index) {
    int at = index(0);
    double best = tab[at];
    for (int t = 1; t < cnt; ++t) {
        const int r = index(t);
        const double x = tab[r];
        if (x > best) { best = x; at = r; }
    }
    return at;
}

extern __shared__ double jt_lds[];

// the state of one evidence set: potentials | separators | a region of N doubles | scales, in LDS or in slice `slot` of scratch.
// The region holds what the kernel reads out last (unnormalised marginals, family totals), and before that a max run's picks.
struct JtView {
    double *pot, *sep, *reg, *scl;
};
template <bool kLds>
__device__ __forceinline__ JtView jt_view(const JtTables& a, double* scratch, int slot) {
    double* const pot = kLds ? jt_lds : scratch + size_t(slot) * size_t(a.state_cells);
    double* const sep = pot + a.pot_cells;
    double* const reg = sep + a.sep_cells;
    return {pot, sep, reg, reg + a.N};
}

// psi = psi0 x the factors of the clique's home nodes, ascending node id; a barrier behind.  factor(v, node, digit) multiplies v by
// the node's factor at digit(), the node's state in the entry, where the node has one.
template <class F>
__device__ __forceinline__ void jt_potentials(const JtTables& a, double* pot, const int tid, const int nt, F factor) {
    for (int g = tid; g < a.pot_cells; g += nt) {
        const JtClique q = a.cliques[a.ent_clique[g]];
        const int e = g - q.pot_off;
        double v = a.psi0[g];
        for (int h = q.home_lo; h < q.home_hi; ++h) {
            const int node = a.home_nodes[h];
            factor(v, node, [&]() {
                const JtNode nd = a.nodes[node];
                return (e / nd.stride) % nd.k;
            });
        }
        pot[g] = v;
    }
    __syncthreads();
}

// a set's likelihood vectors as a source of factors: where every node's evidence vector starts (slot's words of ev_slot, -1: none)
// and the values; two barriers
struct JtEvidence {
    const int32_t* at;
    const double* val;
};
__device__ __forceinline__ JtEvidence jt_evidence(const JtArgs& a, const int slot, const int set, const int tid, const int nt) {
    int32_t* const evs = a.ev_slot + size_t(slot) * size_t(a.t.n);
    const int32_t* meta = a.ev_meta + 8 * set;
    const int ne = meta[0];
    const int32_t* ev_node = a.ev_node + meta[1];
    const int32_t* ev_off = a.ev_off + meta[2];
    for (int v = tid; v < a.t.n; v += nt) evs[v] = -1;
    __syncthreads();
    for (int j = tid; j < ne; j += nt) evs[ev_node[j]] = ev_off[j];
    __syncthreads();
    return {evs, a.ev_val + meta[3]};
}

// collect and distribute (bn_jt.hpp) over the state of one evidence set.  In: the potentials, a barrier behind them.  Out: every
// clique's table proportional to P(clique, e) (JtMax: to its max-marginal), the scales; a barrier behind.  Three barriers per collect
// level but the last, which has two; two per distribute level.
// JtMax also decodes: pick[c], an entry index per clique, in the state's region (nc int32; nc <= n <= N doubles, idle until the
// read-out), and from the picks `states`.  The decode rides phases that are there anyway: a root's pick the level-0 scale phase (its
// entries are final by then); a level's picks the phase that computes its ratios -- they read the level's entries as collect left
// them and the parents' picks of the phase before, and take their lanes from the far end of the workgroup, so that they share no
// wave with the ratio lanes where the level is narrow; the states the last level's multiply.  Only a forest of roots (one level, no
// distribute) pays a barrier for its states.
template <class Op>
__device__ __forceinline__ void jt_walk(const JtTables& a, const JtView& s, int32_t* states, const int tid, const int nt) {
    double* const pot = s.pot;
    double* const sep = s.sep;
    double* const scl = s.scl;
    int32_t* const pick = reinterpret_cast<int32_t*>(s.reg);
    auto write_states = [&]() {
        for (int v = tid; v < a.n; v += nt) {
            const JtNode nd = a.nodes[v];
            states[v] = (pick[nd.home] / nd.stride) % nd.k;
        }
    };
    // ---- collect: deepest level first
    for (int l = a.nlev - 1; l >= 0; --l) {
        const JtLevel L = a.levels[l];
        for (int gs = L.sep_lo + tid; gs < L.sep_hi; gs += nt) {
            const JtClique q = a.cliques[a.sep_clique[gs]];
            sep[gs] = Op::fold(q.cres_cnt, gathered(pot + q.pot_off + a.c_base[gs], a.c_res + q.cres_off));
        }
        __syncthreads();
        for (int c = L.c_lo + tid; c < L.c_hi; c += nt) {
            const JtClique q = a.cliques[c];
            scl[c] = Op::scale(q.sep_size, [&](int j) { return sep[q.sep_off + j]; });
            if constexpr (Op::kDecode) {
                if (l == 0) pick[c] = first_largest(pot + q.pot_off, q.size, [](int i) { return i; });
            }
        }
        __syncthreads();
        if (l == 0) break;
        const JtLevel U = a.levels[l - 1];
        for (int g = U.pot_lo + tid; g < U.pot_hi; g += nt) {
            const JtClique q = a.cliques[a.ent_clique[g]];
            const int e = g - q.pot_off;
            double v = pot[g];
            for (int c = q.child_lo; c < q.child_hi; ++c) {
                const JtClique ch = a.cliques[c];
                double m = sep[ch.sep_off + a.up_map[ch.up_off + e]];
                const double sc = scl[c];
                if (sc > 0.0) m = m / sc;
                v *= m;
            }
            pot[g] = v;
        }
        __syncthreads();
    }
    if constexpr (Op::kDecode) {
        if (a.nlev == 1) {   // roots only
            write_states();
            __syncthreads();
        }
    }
    // ---- distribute: top level first
    for (int l = 1; l < a.nlev; ++l) {
        const JtLevel L = a.levels[l];
        for (int gs = L.sep_lo + tid; gs < L.sep_hi; gs += nt) {
            const int c = a.sep_clique[gs];
            const JtClique q = a.cliques[c];
            const double nw = Op::fold(q.pres_cnt, gathered(pot + a.cliques[q.parent].pot_off + a.p_base[gs], a.p_res + q.pres_off));
            double m = sep[gs];
            const double sc = scl[c];
            if (sc > 0.0) m = m / sc;
            sep[gs] = m == 0.0 ? 0.0 : nw / m;
        }
        if constexpr (Op::kDecode) {
            for (int c = L.c_hi - 1 - (nt - 1 - tid); c >= L.c_lo; c -= nt) {
                const JtClique q = a.cliques[c];
                const int base = a.c_base[q.sep_off + a.up_map[q.up_off + pick[q.parent]]];
                const int32_t* res = a.c_res + q.cres_off;
                pick[c] = base + first_largest(pot + q.pot_off + base, q.cres_cnt, [&](int t) { return res[t]; });
            }
        }
        __syncthreads();
        for (int g = L.pot_lo + tid; g < L.pot_hi; g += nt) {
            const JtClique q = a.cliques[a.ent_clique[g]];
            pot[g] = pot[g] * sep[q.sep_off + a.dn_map[g]];
        }
        if constexpr (Op::kDecode) {
            if (l == a.nlev - 1) write_states();
        }
        __syncthreads();
    }
}

// read-out: u[x] = the fold of the home clique's entries with x_v = x into the region, a barrier, then set `set`'s beliefs (JtMax:
// max-marginals) u[x] / (u[0] + u[1] + ... left to right from +0.0) and its scales
template <class Op>
__device__ __forceinline__ void jt_read_out(const JtArgs& a, const JtView& s, const int set, const int tid, const int nt) {
    const JtTables& t = a.t;
    for (int i = tid; i < t.N; i += nt) {
        const JtNode nd = t.nodes[t.elem_node[i]];
        const JtClique q = t.cliques[nd.home];
        const double* tab = s.pot + q.pot_off + (i - nd.bel_off) * nd.stride;
        const int span = nd.stride * nd.k;
        s.reg[i] = Op::fold(q.size / nd.k, [&](int x) { return tab[(x / nd.stride) * span + x % nd.stride]; });
    }
    __syncthreads();
    double* const bel = a.beliefs + size_t(set) * size_t(t.N);
    for (int i = tid; i < t.N; i += nt) {
        const JtNode nd = t.nodes[t.elem_node[i]];
        double tot = 0.0;
        for (int x = 0; x < nd.k; ++x) tot += s.reg[nd.bel_off + x];
        bel[i] = s.reg[i] / tot;
    }
    double* const out = a.scales + size_t(set) * size_t(t.nc);
    for (int c = tid; c < t.nc; c += nt) out[c] = s.scl[c];
}

// a run of one evidence set per workgroup: workgroup b runs set set_base + b in state slot b
template <class Op, bool kLds>
__device__ __forceinline__ void jt_run(const JtArgs& a) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int slot = blockIdx.x, set = a.set_base + slot;
    const JtView s = jt_view<kLds>(a.t, a.scratch, slot);
    const JtEvidence ev = jt_evidence(a, slot, set, tid, nt);
    jt_potentials(a.t, s.pot, tid, nt, [&](double& v, int node, auto digit) {
        const int at = ev.at[node];
        if (at >= 0) v *= ev.val[at + digit()];
    });
    jt_walk<Op>(a.t, s, Op::kDecode ? a.states + size_t(set) * size_t(a.t.n) : nullptr, tid, nt);
    jt_read_out<Op>(a, s, set, tid, nt);
}

template <bool kLds>
__global__ void __launch_bounds__(kLds ? kJtLdsThreads : kJtMemThreads) jt_kernel(JtArgs a) {
    jt_run<JtSum, kLds>(a);
}

// max-propagation with backtracking (bn_jt.hpp, "Exact MPE")
template <bool kLds>
__global__ void __launch_bounds__(kLds ? kJtLdsThreads : kJtMemThreads) jt_mpe_kernel(JtArgs a) {
    jt_run<JtMax, kLds>(a);
}

// ---- exact expectation-maximisation (bn_jt.hpp, "Exact EM"): the sum run of one pattern row -- evidence from the row's bytes --
// and, from the tables distribute leaves, the family posteriors of every CPT into the launch's slice of `b`.  The state is that of
// jt_kernel; the region of the unnormalised marginals holds the n family totals.  No atomics, nothing shared between workgroups.
template <bool kLds>
__global__ void __launch_bounds__(kLds ? kJtLdsThreads : kJtMemThreads) jt_em_kernel(JtEmArgs a) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int row = blockIdx.x;
    const JtView s = jt_view<kLds>(a.t, a.scratch, row);
    double* const tot = s.reg;   // [n] of the region's N
    const uint8_t* const pat = a.patterns + size_t(row) * size_t(a.t.n);

    // the one-hot vectors of the observed nodes
    jt_potentials(a.t, s.pot, tid, nt, [&](double& v, int node, auto digit) {
        const int cell = pat[node];
        if (cell != kJtEmMissing) v *= digit() == cell ? 1.0 : 0.0;
    });
    jt_walk<JtSum>(a.t, s, nullptr, tid, nt);
    // ---- family read-out: u[q], flat CPT order
    double* const out = a.b + size_t(row) * size_t(a.S);
    for (int q = tid; q < a.S; q += nt) {
        const JtFamily F = a.families[a.f_node[q]];
        out[q] = sum_two_level(s.pot + F.pot_off + a.f_base[q], a.f_res + F.res_off, F.res_cnt);
    }
    __syncthreads();
    // s_v: one lane per node, its entries in flat order
    for (int v = tid; v < a.t.n; v += nt) {
        const JtFamily F = a.families[v];
        const double* u = out + F.cpt_lo;
        tot[v] = two_level_sum(F.cpt_cnt, [&](int t) { return u[t]; });
    }
    __syncthreads();
    for (int q = tid; q < a.S; q += nt) {
        const double sv = tot[a.f_node[q]];
        out[q] = sv > 0.0 ? out[q] / sv : 0.0;   // false for zero and for NaN: the family contributes nothing
    }
    // the row's skipped families and log-likelihood: the first wave, reduced across its lanes (no stated order)
    if (tid < 64) {
        int skipped = 0;
        for (int v = tid; v < a.t.n; v += 64) skipped += tot[v] > 0.0 ? 0 : 1;
        double ll = 0.0;
        for (int c = tid; c < a.t.nc; c += 64) ll += log(s.scl[c]);
        for (int off = 32; off > 0; off >>= 1) {
            skipped += __shfl_down(skipped, off, 64);
            ll += __shfl_down(ll, off, 64);
        }
        if (tid == 0) {
            a.skipped[row] = skipped;
            a.loglik[row] = ll;
        }
    }
}

// L = sum_p (count_p > 0 ? double(count_p) x ll_p : 0.0) and the skipped families of one E-step: one workgroup over the table
__global__ void __launch_bounds__(256) jt_em_total_kernel(JtEmTotalArgs a) {
    __shared__ double s_l[256];
    __shared__ unsigned long long s_k[256];
    const int tid = threadIdx.x;
    double l = 0.0;
    unsigned long long k = 0;
    for (int64_t p = tid; p < a.n_patterns; p += 256) {
        const unsigned long long c = a.counts[p];
        if (c > 0) l += double(c) * a.loglik[p];
        k += (unsigned long long)a.skipped[p];
    }
    s_l[tid] = l;
    s_k[tid] = k;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { s_l[tid] += s_l[tid + h]; s_k[tid] += s_k[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) {
        *a.L = s_l[0];
        *a.skipped_total += s_k[0];
    }
}

// one workgroup per set (row) of `blocks`: the state in LDS (form 1) or in the arguments' scratch (form 2)
template <class Args>
int launch_form(void (*lds)(Args), void (*mem)(Args), const Args& a, int form, int blocks, void* stream) {
    return launched([&] {
        if (form == 1) hipLaunchKernelGGL(lds, dim3(blocks), dim3(kJtLdsThreads), size_t(a.t.state_cells) * sizeof(double), (hipStream_t)stream, a);
        else hipLaunchKernelGGL(mem, dim3(blocks), dim3(kJtMemThreads), 0, (hipStream_t)stream, a);
    });
}

}  // namespace

int launch_jt_base(const JtBaseArgs& a, void* stream) {
    return launched([&] {
        if (a.pot_cells > 0) hipLaunchKernelGGL(jt_base_kernel, dim3((a.pot_cells + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    });
}

int launch_jt(const JtArgs& a, int form, int kind, int n_sets, void* stream) {
    return kind == kJtSum ? launch_form(jt_kernel<true>, jt_kernel<false>, a, form, n_sets, stream)
                          : launch_form(jt_mpe_kernel<true>, jt_mpe_kernel<false>, a, form, n_sets, stream);
}

int launch_jt_em(const JtEmArgs& a, int form, int n_rows, void* stream) {
    return launch_form(jt_em_kernel<true>, jt_em_kernel<false>, a, form, n_rows, stream);
}

int launch_jt_em_total(const JtEmTotalArgs& a, void* stream) {
    return launched([&] { hipLaunchKernelGGL(jt_em_total_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a); });
}

}  // namespace bnmi
