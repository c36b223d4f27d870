// bn_small_evidence.inc -- a set's evidence (:68-73) from the caller's arrays themselves (mapped host memory) into the initial state in
// LDS, and the rest of the node vectors from npi_init / 1.0 (s == 0) or from `state`, where an earlier launch left the run -- as TEXT,
// included by bp_small_kernel (bn_small.hip, ev_mode != 0) and mpe_small_kernel (bn_maxprod.hip).  (A __forceinline__ function of the
// same statements gives bp_small_kernel<1> 73 vector registers instead of 69.)  Nodes, offsets AND values are requested together --
// the values' range is known from the set's header, so they travel while the initial state is written and wait in the staging array
// until the offsets say where they belong (one trip over PCIe instead of two dependent ones).
// In scope where it is included: SmallLds L; the kernel's arguments `a` (N, M, T, npi_init, node_off); int tid, nt, s, c0 (= s & 1);
// const double* state; and the set's evidence, declared immediately above the include: int ne, nval; const int32_t* ev_node, *ev_off;
// const double* ev_val.  The staging array has been zeroed by every thread's loop above, and is zero again behind.
int v0 = 0, o0 = 0;
double x0 = 0.0;
if (tid < ne) { v0 = ev_node[tid]; o0 = ev_off[tid]; }
if (tid < nval && s == 0) x0 = ev_val[tid];
for (int y = tid; y < a.N; y += nt) {
    L.frz[y] = 0;
    L.npi[c0 * a.N + y] = s == 0 ? a.npi_init[y] : state[2 * a.M + y];
    L.nlam[c0 * a.N + y] = s == 0 ? 1.0 : state[2 * a.M + a.N + y];
}
__syncthreads();   // (the staging array has been zeroed by every thread's loop above)
const bool vals_in_lds = nval <= a.T;
if (s == 0 && vals_in_lds)
    for (int t = tid; t < nval; t += nt) L.stg[t] = t == tid ? x0 : ev_val[t];
__syncthreads();
for (int j = tid; j < ne; j += nt) {  // both pi(v) and lambda(v) take the evidence vector (:68-73)
    const int v = j == tid ? v0 : ev_node[j], o = j == tid ? o0 : ev_off[j];
    const int lo = a.node_off[v], hi = a.node_off[v + 1];
    for (int i = 0; i < hi - lo; ++i) {
        L.frz[lo + i] = 1;
        if (s == 0) {
            const double x = vals_in_lds ? L.stg[o + i] : ev_val[o + i];
            L.npi[c0 * a.N + lo + i] = x;
            L.nlam[c0 * a.N + lo + i] = x;
        }
    }
}
__syncthreads();
if (s == 0 && vals_in_lds)
    for (int t = tid; t < nval; t += nt) L.stg[t] = 0.0;  // the padding of the runs is zero again
