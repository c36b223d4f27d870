// bn_small_items.inc -- this thread's work items of the one-workgroup path (bn_small.hpp / bn_small_plan.cpp), kept in registers for the
// whole run, and what the wave needs to know of its lanes' items -- as TEXT, included at the top of bp_small_kernel (bn_small.hip) and
// of em_small_kernel (bn_em.hip) in front of bn_small_sweep.inc, which names these arrays.  ROUNDS = items of one kind per thread (1,
// 2 or kSmallMaxRounds): a network that fits one round keeps a third of the registers.
// In scope where it is included: the template parameter ROUNDS, the kernel's arguments `a` (re, rb, rc, ent, ent_cpt, bslot, cslot,
// term), int tid, nt.
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
    if (r < a.re) { ent[r] = a.ent[r * nt + tid]; ecpt[r] = a.ent_cpt[r * nt + tid]; }
    if (r < a.rb) bs[r] = a.bslot[r * nt + tid];
    if (r < a.rc) cs[r] = a.cslot[r * nt + tid];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        treg[r][j] = 0u;
        if (kTermsInRegs && ((ent[r].y >> 24) & 1u) && j < int((ent[r].y >> 16) & 0xffu)) treg[r][j] = a.term[(ent[r].y & 0xffffu) + j];
    }
    e_mm[r] = wave_imax(((ent[r].y >> 24) & 1u) ? int((ent[r].y >> 16) & 0xffu) : 0);
    b_rmax[r] = wave_imax(int(bs[r].x >> 16));
    b_kmax[r] = wave_imax(bs[r].z != 0 ? int((bs[r].y >> 16) & 0xffu) : 0);
    c_dmax[r] = wave_imax(int(cs[r].x >> 16));
    c_kmax[r] = wave_imax((cs[r].z & 0xffu) != 0 ? int((cs[r].y >> 16) & 0xffu) : 0);
}
