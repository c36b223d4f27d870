// bn_small_items.inc -- this thread's work items (bn_small.hpp / bn_small_plan.cpp), kept in registers for the whole run, and what the
// wave needs to know of its lanes' items -- as TEXT, included by bp_small_kernel (bn_small.hip) and em_small_kernel (bn_em.hip) in front
// of bn_small_sweep.inc, which names these arrays, and by bp_mid_kernel (bn_mid.hip) and mpe_mid_kernel (bn_maxprod.hip) in front of
// their own sweeps.  (mpe_small_kernel keeps items of its own, MpeItems: bn_maxprod.hip says why.)  ROUNDS = items of one kind per thread (1, 2 or
// kSmallMaxRounds): a network that fits one round keeps a third of the registers.
// In scope where it is included: the template parameter ROUNDS, int tid, and these locals, declared immediately above the include:
//   it_ent, it_cpt, it_bslot, it_cslot, it_term   the tables' bases (a workgroup of several: its part's offsets added)
//   it_nt                                          the tables' stride from round to round
//   it_mine                                        this thread has items (a launch is as wide as its widest part)
//   it_re, it_rb, it_rc                            rounds of entry, accumulator and product items to load (0: that kind stays empty)
SmallEntry ent[ROUNDS];
double ecpt[ROUNDS];
SmallSlot bs[ROUNDS], cs[ROUNDS];
constexpr bool kTermsInRegs = ROUNDS == 1;
uint32_t treg[ROUNDS][4];
int e_mm[ROUNDS], b_rmax[ROUNDS], b_kmax[ROUNDS], c_dmax[ROUNDS], c_kmax[ROUNDS];
#pragma unroll
for (int r = 0; r < ROUNDS; ++r) {
    ent[r] = SmallEntry{0u, 0u}; ecpt[r] = 0.0;
    bs[r] = SmallSlot{0u, 0u, 0u, 0u}; cs[r] = SmallSlot{0u, 0u, 0u, 0u};
    if (it_mine && r < it_re) { ent[r] = it_ent[r * it_nt + tid]; ecpt[r] = it_cpt[r * it_nt + tid]; }
    if (it_mine && r < it_rb) bs[r] = it_bslot[r * it_nt + tid];
    if (it_mine && r < it_rc) cs[r] = it_cslot[r * it_nt + tid];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        treg[r][j] = 0u;
        if (kTermsInRegs && ((ent[r].y >> 24) & 1u) && j < int((ent[r].y >> 16) & 0xffu)) treg[r][j] = it_term[(ent[r].y & 0xffffu) + j];
    }
    e_mm[r] = wave_imax(((ent[r].y >> 24) & 1u) ? int((ent[r].y >> 16) & 0xffu) : 0);
    b_rmax[r] = wave_imax(int(bs[r].x >> 16));
    b_kmax[r] = wave_imax(bs[r].z != 0 ? int((bs[r].y >> 16) & 0xffu) : 0);
    c_dmax[r] = wave_imax(int(cs[r].x >> 16));
    c_kmax[r] = wave_imax((cs[r].z & 0xffu) != 0 ? int((cs[r].y >> 16) & 0xffu) : 0);
}
