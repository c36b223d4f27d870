// bn_jt.hip -- junction-tree propagation on gfx950: the base potentials, and the two-pass run of one evidence set per workgroup
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

}  // namespace

int launch_jt_base(const JtBaseArgs& a, void* stream) {
    (void)hipGetLastError();  // drop any stale error of this thread
    if (a.pot_cells > 0) hipLaunchKernelGGL(jt_base_kernel, dim3((a.pot_cells + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

int launch_jt(const JtArgs& a, int form, int n_sets, void* stream) {
    (void)hipGetLastError();
    if (form == 1) hipLaunchKernelGGL(jt_kernel<true>, dim3(n_sets), dim3(kJtLdsThreads), size_t(a.state_cells) * sizeof(double), (hipStream_t)stream, a);
    else hipLaunchKernelGGL(jt_kernel<false>, dim3(n_sets), dim3(kJtMemThreads), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace bnmi
