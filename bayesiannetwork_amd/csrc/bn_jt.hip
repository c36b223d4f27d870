// bn_jt.hip -- junction-tree propagation on gfx950: the base potentials, and the two-pass run of one evidence set per workgroup,
// as a sum run (jt_kernel: marginals), as a max run (jt_mpe_kernel: exact MPE) and as the E-step of exact expectation-maximisation
// (jt_em_kernel: the sum run of a pattern row and its family posteriors, with the small kernels of its sums and its M-step)
// (rules: bn_jt.hpp; item tables: bn_jt_plan.hpp).  The same item code runs over LDS (form 1) and over the set's slice of device
// scratch (form 2): the kernel is a template over where the state lives, so the compiler sees the address space.  A workgroup
// reads and writes its own state only; every phase ends in __syncthreads(), and no lane waits on anything else.
#include <hip/hip_runtime.h>

#include "bn_jt.hpp"

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

// two-level sum (bn_jt.hpp) of tab[res[0]], tab[res[1]], ...
template <class P>
__device__ inline double sum_two_level(P tab, const int32_t* res, int cnt) {
    double total = 0.0;
    for (int r = 0; r < cnt; r += kJtRun) {
        const int hi = r + kJtRun < cnt ? r + kJtRun : cnt;
        double run = 0.0;
        for (int t = r; t < hi; ++t) run += tab[res[t]];
        total += run;
    }
    return total;
}

// collect and distribute of a sum run (bn_jt.hpp) over the state of one evidence set: the one text of jt_kernel and jt_em_kernel.
// In: the potentials, a barrier behind them.  Out: every clique's table proportional to P(clique, e), the scales; a barrier behind.
template <class Args, class P>
__device__ __forceinline__ void jt_walk(const Args& a, P pot, P sep, P scl, const int tid, const int nt) {
    // ---- collect: deepest level first
    for (int l = a.nlev - 1; l >= 0; --l) {
        const JtLevel L = a.levels[l];
        for (int gs = L.sep_lo + tid; gs < L.sep_hi; gs += nt) {
            const JtClique q = a.cliques[a.sep_clique[gs]];
            sep[gs] = sum_two_level(pot + q.pot_off + a.c_base[gs], a.c_res + q.cres_off, q.cres_cnt);
        }
        __syncthreads();
        for (int c = L.c_lo + tid; c < L.c_hi; c += nt) {
            const JtClique q = a.cliques[c];
            double s = 0.0;
            for (int j = 0; j < q.sep_size; ++j) s += sep[q.sep_off + j];
            scl[c] = s;
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
                const double s = scl[c];
                if (s > 0.0) m = m / s;
                v *= m;
            }
            pot[g] = v;
        }
        __syncthreads();
    }
    // ---- distribute: top level first
    for (int l = 1; l < a.nlev; ++l) {
        const JtLevel L = a.levels[l];
        for (int gs = L.sep_lo + tid; gs < L.sep_hi; gs += nt) {
            const int c = a.sep_clique[gs];
            const JtClique q = a.cliques[c];
            const double nw = sum_two_level(pot + a.cliques[q.parent].pot_off + a.p_base[gs], a.p_res + q.pres_off, q.pres_cnt);
            double m = sep[gs];
            const double s = scl[c];
            if (s > 0.0) m = m / s;
            sep[gs] = m == 0.0 ? 0.0 : nw / m;
        }
        __syncthreads();
        for (int g = L.pot_lo + tid; g < L.pot_hi; g += nt) {
            const JtClique q = a.cliques[a.ent_clique[g]];
            pot[g] = pot[g] * sep[q.sep_off + a.dn_map[g]];
        }
        __syncthreads();
    }
}

extern __shared__ double jt_lds[];

template <bool kLds>
__global__ void __launch_bounds__(kLds ? kJtLdsThreads : kJtMemThreads) jt_kernel(JtArgs a) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int slot = blockIdx.x, set = a.set_base + slot;
    double* const st = kLds ? jt_lds : a.scratch + size_t(slot) * size_t(a.state_cells);
    double* const pot = st;
    double* const sep = pot + a.pot_cells;
    double* const marg = sep + a.sep_cells;
    double* const scl = marg + a.N;
    int32_t* const evs = a.ev_slot + size_t(slot) * size_t(a.n);
    const int32_t* meta = a.ev_meta + 8 * set;
    const int ne = meta[0];
    const int32_t* ev_node = a.ev_node + meta[1];
    const int32_t* ev_off = a.ev_off + meta[2];
    const double* ev_val = a.ev_val + meta[3];

    // where every node's evidence vector starts
    for (int v = tid; v < a.n; v += nt) evs[v] = -1;
    __syncthreads();
    for (int j = tid; j < ne; j += nt) evs[ev_node[j]] = ev_off[j];
    __syncthreads();
    // psi = psi0 x the evidence of the clique's home nodes, ascending node id
    for (int g = tid; g < a.pot_cells; g += nt) {
        const JtClique q = a.cliques[a.ent_clique[g]];
        const int e = g - q.pot_off;
        double v = a.psi0[g];
        for (int h = q.home_lo; h < q.home_hi; ++h) {
            const int node = a.home_nodes[h];
            const int at = evs[node];
            if (at >= 0) {
                const JtNode nd = a.nodes[node];
                v *= ev_val[at + (e / nd.stride) % nd.k];
            }
        }
        pot[g] = v;
    }
    __syncthreads();
    jt_walk(a, pot, sep, scl, tid, nt);
    // ---- read-out
    for (int i = tid; i < a.N; i += nt) {
        const JtNode nd = a.nodes[a.elem_node[i]];
        const JtClique q = a.cliques[nd.home];
        const double* tab = pot + q.pot_off + (i - nd.bel_off) * nd.stride;
        const int cnt = q.size / nd.k, span = nd.stride * nd.k;
        double total = 0.0;
        for (int r = 0; r < cnt; r += kJtRun) {
            const int hi = r + kJtRun < cnt ? r + kJtRun : cnt;
            double run = 0.0;
            for (int t = r; t < hi; ++t) run += tab[(t / nd.stride) * span + t % nd.stride];
            total += run;
        }
        marg[i] = total;
    }
    __syncthreads();
    double* const bel = a.beliefs + size_t(set) * size_t(a.N);
    for (int i = tid; i < a.N; i += nt) {
        const JtNode nd = a.nodes[a.elem_node[i]];
        double tot = 0.0;
        for (int x = 0; x < nd.k; ++x) tot += marg[nd.bel_off + x];
        bel[i] = marg[i] / tot;
    }
    double* const out = a.scales + size_t(set) * size_t(a.nc);
    for (int c = tid; c < a.nc; c += nt) out[c] = scl[c];
}

// ---- exact expectation-maximisation (bn_jt.hpp, "Exact EM"): the sum run of one pattern row -- evidence from the row's bytes --
// and, from the tables distribute leaves, the family posteriors of every CPT into the launch's slice of `b`.  The state is that of
// jt_kernel; the region of the unnormalised marginals holds the n family totals.  No atomics, nothing shared between workgroups.
template <bool kLds>
__global__ void __launch_bounds__(kLds ? kJtLdsThreads : kJtMemThreads) jt_em_kernel(JtEmArgs a) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int row = blockIdx.x;
    double* const st = kLds ? jt_lds : a.scratch + size_t(row) * size_t(a.state_cells);
    double* const pot = st;
    double* const sep = pot + a.pot_cells;
    double* const tot = sep + a.sep_cells;   // [n] of the region's N
    double* const scl = tot + a.N;
    const uint8_t* const pat = a.patterns + size_t(row) * size_t(a.n);

    // psi = psi0 x the one-hot vectors of the clique's observed home nodes, ascending node id
    for (int g = tid; g < a.pot_cells; g += nt) {
        const JtClique q = a.cliques[a.ent_clique[g]];
        const int e = g - q.pot_off;
        double v = a.psi0[g];
        for (int h = q.home_lo; h < q.home_hi; ++h) {
            const int node = a.home_nodes[h];
            const int cell = pat[node];
            if (cell != kJtEmMissing) {
                const JtNode nd = a.nodes[node];
                v *= (e / nd.stride) % nd.k == cell ? 1.0 : 0.0;
            }
        }
        pot[g] = v;
    }
    __syncthreads();
    jt_walk(a, pot, sep, scl, tid, nt);
    // ---- family read-out: u[q], flat CPT order
    double* const out = a.b + size_t(row) * size_t(a.S);
    for (int q = tid; q < a.S; q += nt) {
        const JtFamily F = a.families[a.f_node[q]];
        out[q] = sum_two_level(pot + F.pot_off + a.f_base[q], a.f_res + F.res_off, F.res_cnt);
    }
    __syncthreads();
    // s_v: one lane per node, its entries in flat order
    for (int v = tid; v < a.n; v += nt) {
        const JtFamily F = a.families[v];
        const double* u = out + F.cpt_lo;
        double total = 0.0;
        for (int r = 0; r < F.cpt_cnt; r += kJtRun) {
            const int hi = r + kJtRun < F.cpt_cnt ? r + kJtRun : F.cpt_cnt;
            double run = 0.0;
            for (int t = r; t < hi; ++t) run += u[t];
            total += run;
        }
        tot[v] = total;
    }
    __syncthreads();
    for (int q = tid; q < a.S; q += nt) {
        const double s = tot[a.f_node[q]];
        out[q] = s > 0.0 ? out[q] / s : 0.0;   // false for zero and for NaN: the family contributes nothing
    }
    // the row's skipped families and log-likelihood: the first wave, reduced across its lanes (no stated order)
    if (tid < 64) {
        int skipped = 0;
        for (int v = tid; v < a.n; v += 64) skipped += tot[v] > 0.0 ? 0 : 1;
        double ll = 0.0;
        for (int c = tid; c < a.nc; c += 64) ll += log(scl[c]);
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

// the M-step of bn_em.hpp (em_mstep_kernel's arithmetic) on the flat array alone: one thread per CPT entry
__global__ void __launch_bounds__(256) jt_em_mstep_kernel(JtEmMstepArgs a) {
    const int q = int(blockIdx.x * blockDim.x + threadIdx.x);
    double d = 0.0;
    if (q < a.S) {
        const JtFamily F = a.families[a.f_node[q]];
        const int k = a.nodes[a.f_node[q]].k;
        const int first = F.cpt_lo + (q - F.cpt_lo) / k * k;
        double tot = 0.0;
        for (int i = 0; i < k; ++i) tot += a.E[first + i] + a.prior;
        const double th = tot > 0.0 ? (a.E[q] + a.prior) / tot : 1.0 / double(k);
        d = fabs(th - a.theta[q]);
        a.theta[q] = th;
    }
    // md = (md < d) ? d : md from +0.0: a NaN never enters; the bit patterns of the rest order like the values
    unsigned long long bits = (unsigned long long)__double_as_longlong(0.0 < d ? d : 0.0);
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(bits, off, 64);
        bits = bits < o ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(a.delta_bits, bits);
}

// ---- max-propagation with backtracking (bn_jt.hpp, "Exact MPE"): the walk of jt_kernel with every sum replaced by the max fold,
// and the pick of one entry per clique on the way down.  The picks (nc int32) live in the state's region of the unnormalised
// marginals (N >= n >= nc doubles), idle until the read-out: the state is that of jt_kernel, and the states are written from the
// picks in the last phase before the read-out fills the region.

// max fold (bn_jt.hpp) of tab[res[0]], tab[res[1]], ...
template <class P>
__device__ inline double max_fold(P tab, const int32_t* res, int cnt) {
    double acc = 0.0;
    for (int t = 0; t < cnt; ++t) {
        const double x = tab[res[t]];
        acc = acc < x ? x : acc;
    }
    return acc;
}

template <bool kLds>
__global__ void __launch_bounds__(kLds ? kJtLdsThreads : kJtMemThreads) jt_mpe_kernel(JtArgs a) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int slot = blockIdx.x, set = a.set_base + slot;
    double* const st = kLds ? jt_lds : a.scratch + size_t(slot) * size_t(a.state_cells);
    double* const pot = st;
    double* const sep = pot + a.pot_cells;
    double* const marg = sep + a.sep_cells;
    double* const scl = marg + a.N;
    int32_t* const evs = a.ev_slot + size_t(slot) * size_t(a.n);
    const int32_t* meta = a.ev_meta + 8 * set;
    const int ne = meta[0];
    const int32_t* ev_node = a.ev_node + meta[1];
    const int32_t* ev_off = a.ev_off + meta[2];
    const double* ev_val = a.ev_val + meta[3];

    for (int v = tid; v < a.n; v += nt) evs[v] = -1;
    __syncthreads();
    for (int j = tid; j < ne; j += nt) evs[ev_node[j]] = ev_off[j];
    __syncthreads();
    for (int g = tid; g < a.pot_cells; g += nt) {
        const JtClique q = a.cliques[a.ent_clique[g]];
        const int e = g - q.pot_off;
        double v = a.psi0[g];
        for (int h = q.home_lo; h < q.home_hi; ++h) {
            const int node = a.home_nodes[h];
            const int at = evs[node];
            if (at >= 0) {
                const JtNode nd = a.nodes[node];
                v *= ev_val[at + (e / nd.stride) % nd.k];
            }
        }
        pot[g] = v;
    }
    __syncthreads();
    int32_t* const pick = reinterpret_cast<int32_t*>(marg);   // [nc], nc <= n <= N
    int32_t* const states = a.states + size_t(set) * size_t(a.n);
    // every pick is made: the states, before the read-out overwrites the picks
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
            sep[gs] = max_fold(pot + q.pot_off + a.c_base[gs], a.c_res + q.cres_off, q.cres_cnt);
        }
        __syncthreads();
        for (int c = L.c_lo + tid; c < L.c_hi; c += nt) {
            const JtClique q = a.cliques[c];
            double s = 0.0;
            for (int j = 0; j < q.sep_size; ++j) {
                const double x = sep[q.sep_off + j];
                s = s < x ? x : s;
            }
            scl[c] = s;
            if (l == 0) {   // a root's entries are final: the lowest index of its largest entry
                const double* tab = pot + q.pot_off;
                int at = 0;
                double best = tab[0];
                for (int i = 1; i < q.size; ++i) {
                    const double x = tab[i];
                    if (x > best) { best = x; at = i; }
                }
                pick[c] = at;
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
                const double s = scl[c];
                if (s > 0.0) m = m / s;
                v *= m;
            }
            pot[g] = v;
        }
        __syncthreads();
    }
    if (a.nlev == 1) {   // roots only
        write_states();
        __syncthreads();
    }
    // ---- distribute: top level first.  The picks of a level ride the phase that computes its ratios: they read the level's
    // entries as collect left them and the parents' picks of the phase before, and take the lanes from the far end.  The states
    // ride the last level's multiply.
    for (int l = 1; l < a.nlev; ++l) {
        const JtLevel L = a.levels[l];
        for (int gs = L.sep_lo + tid; gs < L.sep_hi; gs += nt) {
            const int c = a.sep_clique[gs];
            const JtClique q = a.cliques[c];
            const double nw = max_fold(pot + a.cliques[q.parent].pot_off + a.p_base[gs], a.p_res + q.pres_off, q.pres_cnt);
            double m = sep[gs];
            const double s = scl[c];
            if (s > 0.0) m = m / s;
            sep[gs] = m == 0.0 ? 0.0 : nw / m;
        }
        for (int c = L.c_hi - 1 - (nt - 1 - tid); c >= L.c_lo; c -= nt) {
            const JtClique q = a.cliques[c];
            const int base = a.c_base[q.sep_off + a.up_map[q.up_off + pick[q.parent]]];
            const double* tab = pot + q.pot_off + base;
            const int32_t* res = a.c_res + q.cres_off;
            int at = res[0];
            double best = tab[at];
            for (int t = 1; t < q.cres_cnt; ++t) {
                const int r = res[t];
                const double x = tab[r];
                if (x > best) { best = x; at = r; }
            }
            pick[c] = base + at;
        }
        __syncthreads();
        for (int g = L.pot_lo + tid; g < L.pot_hi; g += nt) {
            const JtClique q = a.cliques[a.ent_clique[g]];
            pot[g] = pot[g] * sep[q.sep_off + a.dn_map[g]];
        }
        if (l == a.nlev - 1) write_states();
        __syncthreads();
    }
    // ---- read-out: the max-marginals
    for (int i = tid; i < a.N; i += nt) {
        const JtNode nd = a.nodes[a.elem_node[i]];
        const JtClique q = a.cliques[nd.home];
        const double* tab = pot + q.pot_off + (i - nd.bel_off) * nd.stride;
        const int cnt = q.size / nd.k, span = nd.stride * nd.k;
        double acc = 0.0;
        for (int t = 0; t < cnt; ++t) {
            const double x = tab[(t / nd.stride) * span + t % nd.stride];
            acc = acc < x ? x : acc;
        }
        marg[i] = acc;
    }
    __syncthreads();
    double* const bel = a.beliefs + size_t(set) * size_t(a.N);
    for (int i = tid; i < a.N; i += nt) {
        const JtNode nd = a.nodes[a.elem_node[i]];
        double tot = 0.0;
        for (int x = 0; x < nd.k; ++x) tot += marg[nd.bel_off + x];
        bel[i] = marg[i] / tot;
    }
    double* const out = a.scales + size_t(set) * size_t(a.nc);
    for (int c = tid; c < a.nc; c += nt) out[c] = scl[c];
}

}  // namespace

int launch_jt_base(const JtBaseArgs& a, void* stream) {
    (void)hipGetLastError();  // drop any stale error of this thread
    if (a.pot_cells > 0) hipLaunchKernelGGL(jt_base_kernel, dim3((a.pot_cells + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int launch_jt(const JtArgs& a, int form, int kind, int n_sets, void* stream) {
    (void)hipGetLastError();
    const size_t lds = size_t(a.state_cells) * sizeof(double);
    hipStream_t s = (hipStream_t)stream;
    if (kind == kJtSum) {
        if (form == 1) hipLaunchKernelGGL(jt_kernel<true>, dim3(n_sets), dim3(kJtLdsThreads), lds, s, a);
        else hipLaunchKernelGGL(jt_kernel<false>, dim3(n_sets), dim3(kJtMemThreads), 0, s, a);
    } else {
        if (form == 1) hipLaunchKernelGGL(jt_mpe_kernel<true>, dim3(n_sets), dim3(kJtLdsThreads), lds, s, a);
        else hipLaunchKernelGGL(jt_mpe_kernel<false>, dim3(n_sets), dim3(kJtMemThreads), 0, s, a);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int launch_jt_em(const JtEmArgs& a, int form, int n_rows, void* stream) {
    (void)hipGetLastError();
    hipStream_t s = (hipStream_t)stream;
    if (form == 1) hipLaunchKernelGGL(jt_em_kernel<true>, dim3(n_rows), dim3(kJtLdsThreads), size_t(a.state_cells) * sizeof(double), s, a);
    else hipLaunchKernelGGL(jt_em_kernel<false>, dim3(n_rows), dim3(kJtMemThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int launch_jt_em_total(const JtEmTotalArgs& a, void* stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(jt_em_total_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int launch_jt_em_mstep(const JtEmMstepArgs& a, void* stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(jt_em_mstep_kernel, dim3(unsigned((a.S + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
