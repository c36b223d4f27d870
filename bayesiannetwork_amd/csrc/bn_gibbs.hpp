// bn_gibbs.hpp -- Gibbs sampling with coloured parallel chains (bn_gibbs.hip; the plan: bn_gibbs_plan.hpp; the entry points:
// bn_engine_gibbs.cpp; the host restatement the kernel equals bit for bit: tests/gibbs_refs.py).
//
// The contract (include/bn_mi355x.h states it for the caller):
//   chain c, a 64-bit id, is a Markov chain over the states of all n nodes; hard evidence nodes are clamped.
//   sweep g visits the colours 0, 1, ... and, inside a colour, every node that is not clamped, in slot order -- which equals
//   updating a colour's nodes at once, as the kernel does.
//   one update of node v, fp64, no contraction:  for x = 0 .. k[v] - 1
//       w[x] = cpt_v[row_v][x]  x  cpt_c[row_c(x)][s_c] for every child c of v, ascending child index (one multiply per child)
//       T = w[0] + w[1] + ... left to right (from 0.0)
//       T not a finite number above 0: the state is kept, the chain's `stuck` count goes up by one
//       else t = u x T and the new state is the first x with t < c_x, c_x the same running sum; none: the last x with w[x] > 0
//   u = U x 2^-53, U = (out0 << 21) | (out1 >> 11) of ONE Philox4x32-10 block, counter {v, g, c_lo, c_hi},
//       key {seed_lo, seed_hi ^ 0x47494253}: a pure function of (seed, c, g, v)
//   after sweep g with g >= burn_in and (g - burn_in) % thin == 0 every node's state (clamped nodes too) adds 1 to
//       counts[node_off[v] + state], unsigned 64-bit
// The kernel: a chain is a group of 8, 16, 32 or 64 neighbouring lanes of a wave (GibbsPlan::lanes_per_chain: what covers the
// largest colour class), a workgroup of 256 threads runs 256 / lanes of them; a chain's state bytes and the workgroup's histogram
// (32-bit cells) are in LDS; the lanes of a chain take the slots of the colour in hand in strides of their count; a workgroup
// barrier separates the colours; the tables are read from device memory; the histogram is added to the 64-bit one in device
// memory when the launch ends, and the states go back to device memory, where they rest between launches.  A node of at most
// eight states keeps its weights in registers and walks its children once; a larger one computes every weight twice, once for T
// and once for the choice (the same operations, so the same bits): no array of k[v] weights per lane is kept.
#pragma once

#include <cstdint>

#include "bn_gibbs_plan.hpp"

namespace bnmi {

constexpr uint32_t kGibbsKeyTag = 0x47494253u;

struct GibbsArgs {
    int32_t n, cells, n_colours, state_stride;
    int32_t lanes_log2;                 // log2 of GibbsPlan::lanes_per_chain
    const int32_t* colour_ptr;          // [n_colours + 1]
    const GibbsSlot* slots;             // [n]
    const GibbsChild* children;
    const GibbsTerm* terms;
    const double* cpt;                  // flat, reference row order
    const int16_t* clamp;               // [n] the observed state, -1: free
    uint8_t* states;                    // [n_chains][n] in, out
    unsigned long long* counts;         // [cells] added to
    unsigned long long* stuck;          // [1] added to
    uint64_t chain_begin, n_chains;
    uint64_t sweep_begin;
    uint32_t n_sweeps;
    uint64_t burn_in, thin, seed;
};

// blocks = gibbs_blocks(n_chains, GibbsPlan::chains_per_block), lds_bytes = GibbsPlan::lds_bytes; 0 or the hipError_t
int launch_gibbs(const GibbsArgs& a, int64_t blocks, int32_t lds_bytes, void* stream);

}  // namespace bnmi
