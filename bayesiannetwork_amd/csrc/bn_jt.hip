// bn_jt.hip -- junction-tree propagation on gfx950: the base potentials, and the two-pass run of one evidence set per workgroup,
// as a sum run (jt_kernel: marginals) and as a max run (jt_mpe_kernel: exact MPE) (rules: bn_jt.hpp; item tables: bn_jt_plan.hpp).  The same item code runs over LDS (form 1) and over the set's slice of device
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

}  // namespace bnmi
