// bn_ci_orient.hpp -- from a skeleton and its separating sets to a CPDAG, and from a PDAG to a DAG (include/bn_mi355x.h, bn_learn_pc
// and bn_pdag_to_dag).  Pure host code, no HIP: bn_ci_orient.cpp is also compiled alone by tests/cpp/test_ci_orient.cpp.
//
// A mark matrix m [n][n] of uint8: m[a][b] and m[b][a] set: a - b; only m[a][b] set: a -> b.
#pragma once

#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)
namespace bnmi {

// v-structures.  cpdag starts as the skeleton (symmetric).  For every z, x < y in increasing (z, x, y) with x - z, y - z in the skeleton,
// x and y not adjacent, a recorded separating set (sep_len[x * n + y] >= 0) and z not in it: x -> z and y -> z, each unless that edge
// is already oriented the other way (the first orientation wins).  sep_idx [n * n * stride].
void pc_orient_colliders(int32_t n, const uint8_t* skeleton, const int32_t* sep_len, const int32_t* sep_idx, int32_t stride, uint8_t* cpdag);

// Meek's rules R1, R2, R3 to a fixed point.  One scan visits the ordered pairs (a, b) in increasing (a, b); where a - b is undirected
// it becomes a -> b at once if R1 (some c -> a with c, b not adjacent), else R2 (some c with a -> c -> b), else R3 (some c < d, not
// adjacent, with a - c, a - d, c -> b, d -> b) applies.  Scans repeat until one changes nothing.
void pc_meek(int32_t n, uint8_t* cpdag);

// Dor-Tarsi: while nodes remain, take the LOWEST node x that has no outgoing directed edge to a remaining node and whose every
// undirected remaining neighbour is adjacent to every other remaining node adjacent to x; turn its undirected edges towards it and
// remove it.  parents[v] increasing.  False: no such node at some step -- the PDAG has no consistent extension.
bool pdag_to_dag(int32_t n, const uint8_t* pdag, std::vector<std::vector<int32_t>>& parents);

}  // namespace bnmi
#pragma GCC visibility pop
