// bn_learn_terms.hpp -- the term table every device-resident search reads (built by bn_learn_terms.cpp): its limits and the layout
// of its rank tables, for the host and for the kernels.
//
// The term table: per child c, ll(c, S) of every parent set S of at most q nodes other than c, at
//     rank(c, S) = offset[j] + sum over i = 1..j of C(s'_i, i),     S = {s_1 < ... < s_j},  s' = s - (s > c),
//     offset[j] = sum over t < j of C(n - 1, t);   T(n, q) = offset[q + 1] entries per child,  child c's row at c * T.
// A family over the per-family limit holds a quiet NaN: "not eligible".
#pragma once

#include <cstdint>

namespace bnmi {

constexpr int kTermMaxNodes = 64;            // a node has a lane
constexpr int64_t kTermMaxEntries = int64_t(1) << 22;     // n * T(n, q): 32 MiB of terms
// the rank tables as the kernels read them: offset[j], j <= 16, then C(a, i) at [kTermTabBinom + i * 64 + a], i <= 16, a < 64
// (an entry no rank of the table's (n, q) can ask for holds 0)
constexpr int kTermTabBinom = 17;
constexpr int kTermTabWords = kTermTabBinom + 17 * 64;

}  // namespace bnmi
