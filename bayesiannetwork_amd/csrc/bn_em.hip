// bn_em.hip -- expectation-maximisation over the one-workgroup belief-propagation iteration.  The rules (what is added to what, in
// which order): bn_em.hpp.  The iteration itself is bn_small_sweep.inc over bn_small_dev.hpp, the text bp_small_kernel runs: same
// items, same bits.
//
//   em_small_kernel        one workgroup per pattern row.  Evidence from the row's bytes; the sum-product loop with the state in LDS,
//                          bounded by the cap; then the epilogue on the state the run stopped in:
//                            pass 1  entry items: the terms t' of pi(v) into staging (item_entry_any: the iteration's phase 1);
//                            barrier
//                            pass 2  accumulator items of pi(v): r[i] = the run's sum (small_run_sum), r[i] x lambda(v)[i] into the
//                                    idle half of the pi(v) buffer, s = the vector's sum front to back (small_vector_sum), s stored
//                                    in place of every element of the vector;
//                            barrier
//                            pass 3  entry items: b = (t' x lambda(v)[i]) / s -> memory, flat CPT order.
//                          No communication between workgroups, no wait.
//   em_accumulate_kernel   one thread per CPT entry: the chunk's count x b, pattern after pattern, into the sum of the 256-block in
//                          hand; a finished block's sum into E.  The block in hand survives a chunk boundary in `partial`.
//   em_mstep_kernel        one thread per CPT entry: row total, division or the uniform row, |change| -> the maximum (bit patterns of
//                          non-negative doubles order like the values), theta_new into the flat array and, where the caller has them (the
//                          one-workgroup E-step; not the junction tree's, bn_jt.hip), the two device images.
#include "bn_em.hpp"
#include "bn_small_dev.hpp"
#include "bn_item_launch.hpp"
#include "bn_launch.hpp"

namespace bnmi {

#define SMALL_STAMP(k) do { } while (0)   // (bn_small_sweep.inc: the diagnostic clock stamps are bp_small_kernel's)

// ROUNDS = items of one kind per thread (1, 2 or kSmallMaxRounds)
template <int ROUNDS>
__global__ __launch_bounds__(kSmallMaxWaves * kWave) void em_small_kernel(EmSmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) char em_lds[];
    const int set = blockIdx.x;
    const SmallLds L = small_carve(em_lds, a);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const SmallEntry* const it_ent = a.ent; const double* const it_cpt = a.ent_cpt; const uint32_t* const it_term = a.term;
    const SmallSlot* const it_bslot = a.bslot; const SmallSlot* const it_cslot = a.cslot;
    const int it_nt = nt, it_re = a.re, it_rb = a.rb, it_rc = a.rc;
    constexpr bool it_mine = true;
#include "bn_small_items.inc"
    // ---- tables and initial state (:33-73) into LDS; the evidence from the pattern's bytes
    for (int t = tid; t < a.TT; t += nt) L.term[t] = a.term[t];
    for (int t = tid; t < a.CL; t += nt) L.clist[t] = a.clist[t];
    for (int t = tid; t < a.T; t += nt) L.stg[t] = 0.0;  // the padding of the runs stays zero for the whole run
    for (int y = tid; y < a.N; y += nt) {
        L.frz[y] = 0;
        L.npi[y] = a.npi_init[y];
        L.nlam[y] = 1.0;
    }
    for (int x = tid; x < a.M; x += nt) { L.pi[x] = 1.0; L.lam[x] = 1.0; }
    if (tid < 32) L.red[tid] = 0ull;
    __syncthreads();
    const uint8_t* pat = a.patterns + int64_t(set) * a.n;
    for (int v = tid; v < a.n; v += nt) {  // both pi(v) and lambda(v) take the one-hot vector (:68-73)
        const int cell = pat[v];
        if (cell == kEmMissing) continue;
        const int lo = a.node_off[v], hi = a.node_off[v + 1];
        for (int i = 0; i < hi - lo; ++i) {
            const double x = i == cell ? 1.0 : 0.0;
            L.frz[lo + i] = 1;
            L.npi[lo + i] = x;
            L.nlam[lo + i] = x;
        }
    }
    __syncthreads();

    int s = 0, done = 0;
    for (;;) {
#include "bn_small_sweep.inc"
        ++s;
        if (rr < a.eps) { done = 1; break; }          // strict < (:147)
        if (s >= a.max_sweeps) { done = 2; break; }   // the cap: the state is used as it stands
    }

    // ---- the family posteriors of the state the run stopped in (bn_em.hpp, step 3)
    const int fin = s & 1;
    const double* nlam_fin = L.nlam + fin * a.N;
    double* sbuf = L.npi + (fin ^ 1) * a.N;   // the idle half: r[i] x lambda(v)[i], then s
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)   // t' at its place in pi(v)[i]'s run (the lambda-message terms beside it are not read)
        if (r < a.re) item_entry_any<kTermsInRegs, false>(e_mm[r], L.stg, L.term, L.pi + fin * a.M, nlam_fin, ent[r], ecpt[r], treg[r], LdPlain{});
    __syncthreads();
    // (the items of passes 2 and 3 are read from the tables once more, round after round: the registers that held them through the
    // run are free again, and the epilogue runs once)
#pragma unroll 1
    for (int r = 0; r < a.rb; ++r) {
        const SmallSlot q = a.bslot[r * nt + tid];
        const bool on = (q.z & 0xffu) == 1;   // the pi(v) items
        const int out_idx = int(q.y & 0xffffu), k = int((q.y >> 16) & 0xffu), at = lane - int(q.y >> 24);
        const int rmax = wave_imax(int(q.x >> 16)), kmax = wave_imax(q.z != 0 ? k : 0);
        const double ri = small_run_sum(L.stg + int(q.x & 0xffffu), rmax);
        const double val = on ? ri * nlam_fin[out_idx] : 0.0;
        const double sv = small_vector_sum(sbuf, on, out_idx, on ? k : 0, at, val, kmax);
        if (on) sbuf[out_idx] = sv;
    }
    __syncthreads();
    double* out = a.b + int64_t(set) * a.S;
    unsigned skipped = 0;
#pragma unroll 1
    for (int r = 0; r < a.re; ++r) {
        const int32_t flat = a.ent_flat[r * nt + tid];
        if (flat < 0) continue;
        const SmallEntry h = a.ent[r * nt + tid];
        const int idx = int(h.x & 0xffffu);
        const double t = L.stg[h.x >> 16], sv = sbuf[idx];
        const bool ok = sv > 0.0;                 // false for zero and for NaN: the evidence has probability 0 under theta
        out[flat & 0xffff] = ok ? (t * nlam_fin[idx]) / sv : 0.0;
        if (!ok && ((flat >> 16) & 1)) ++skipped;   // counted once per family
    }
    if (skipped) atomicAdd(a.counters + 1, (unsigned long long)skipped);
    if (tid == 0) {
        a.sweeps[set] = s;
        if (done == 2) atomicAdd(a.counters, 1ull);
    }
}

__global__ __launch_bounds__(256) void em_accumulate_kernel(EmAccArgs a) {
    const int q = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= a.S) return;
    double part = a.partial[q], e = a.E[q];
    const double* b = a.b + q;
    for (int32_t j = 0; j < a.chunk; ++j) {
        const int64_t g = a.first + j;
        part += double(a.counts[g]) * b[int64_t(j) * a.S];
        if ((g & (kEmBlock - 1)) == kEmBlock - 1 || g == a.n_patterns - 1) { e += part; part = 0.0; }   // the block is complete
    }
    a.partial[q] = part;
    a.E[q] = e;
}

__global__ __launch_bounds__(256) void em_mstep_kernel(EmMstepArgs a) {
    const int q = int(blockIdx.x * blockDim.x + threadIdx.x);
    double d = 0.0;
    if (q < a.S) {
        const bn_policy::EmRow rw = a.row[q];
        const int first = rw.first, k = rw.k;
        double tot = 0.0;
        for (int i = 0; i < k; ++i) tot += a.E[first + i] + a.prior;
        const double th = tot > 0.0 ? (a.E[q] + a.prior) / tot : 1.0 / double(k);   // (bn_fit_kernels.hip: count / total, else uniform)
        d = fabs(th - a.theta[q]);
        a.theta[q] = th;
        if (a.slot_of) {   // (the junction tree's E-step reads theta itself: no images)
            a.ent_cpt[a.slot_of[q]] = th;
            if (a.init_of[q] >= 0) a.npi_init[a.init_of[q]] = th;
        }
    }
    // md = (md < d) ? d : md from +0.0: a NaN never enters -- it is dropped here, the bit patterns of the rest order like the values
    const unsigned long long bits = wave_umax64_dpp((unsigned long long)__double_as_longlong(res_acc(0.0, d)));
    if ((threadIdx.x & (kWave - 1)) == 0 && bits) atomicMax(a.delta_bits, bits);
}

constexpr auto em_small_of = [](auto R) { return em_small_kernel<decltype(R)::value>; };

int prepare_em_small() { return prepare_item_kernels(em_small_of); }

int launch_em_small(const EmSmallArgs& a, int waves, size_t lds_bytes, int32_t chunk, void* stream) {
    return launch_item_kernel(item_rounds(a.re, a.rb, a.rc), em_small_of, dim3(chunk), dim3(waves * kWave), lds_bytes, stream, a);
}

int launch_em_accumulate(const EmAccArgs& a, void* stream) {
    return launched([&] { hipLaunchKernelGGL(em_accumulate_kernel, dim3(unsigned((a.S + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a); });
}

int launch_em_mstep(const EmMstepArgs& a, void* stream) {
    return launched([&] { hipLaunchKernelGGL(em_mstep_kernel, dim3(unsigned((a.S + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a); });
}

}  // namespace bnmi
