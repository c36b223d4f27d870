// bn_ci_orient.cpp -- the orientation rules of bn_ci_orient.hpp: v-structures from the separating sets, Meek's R1-R3 to a fixed point,
// and the Dor-Tarsi extension of a PDAG.  Pure host code over [n][n] mark matrices.
#include "bn_ci_orient.hpp"

#include <algorithm>

namespace bnmi {

void pc_orient_colliders(int32_t n, const uint8_t* skeleton, const int32_t* sep_len, const int32_t* sep_idx, int32_t stride, uint8_t* cpdag) {
    const size_t N = size_t(n);
    std::copy(skeleton, skeleton + N * N, cpdag);
    for (size_t z = 0; z < N; ++z)
        for (size_t x = 0; x < N; ++x) {
            if (x == z || !skeleton[x * N + z]) continue;
            for (size_t y = x + 1; y < N; ++y) {
                if (y == z || !skeleton[y * N + z] || skeleton[x * N + y]) continue;
                const int32_t len = sep_len[x * N + y];
                if (len < 0) continue;
                const int32_t* s = sep_idx + (x * N + y) * size_t(stride);
                if (std::find(s, s + len, int32_t(z)) != s + len) continue;
                if (cpdag[x * N + z]) cpdag[z * N + x] = 0;   // x -> z unless it is z -> x already
                if (cpdag[y * N + z]) cpdag[z * N + y] = 0;
            }
        }
}

void pc_meek(int32_t n, uint8_t* m) {
    const size_t N = size_t(n);
    auto und = [&](size_t a, size_t b) { return m[a * N + b] && m[b * N + a]; };
    auto dir = [&](size_t a, size_t b) { return m[a * N + b] && !m[b * N + a]; };   // a -> b
    auto adj = [&](size_t a, size_t b) { return m[a * N + b] || m[b * N + a]; };
    for (bool changed = true; changed;) {
        changed = false;
        for (size_t a = 0; a < N; ++a)
            for (size_t b = 0; b < N; ++b) {
                if (a == b || !und(a, b)) continue;
                bool fire = false;
                for (size_t c = 0; c < N && !fire; ++c)   // R1
                    fire = c != a && c != b && dir(c, a) && !adj(c, b);
                for (size_t c = 0; c < N && !fire; ++c)   // R2
                    fire = c != a && c != b && dir(a, c) && dir(c, b);
                for (size_t c = 0; c < N && !fire; ++c) {   // R3
                    if (c == a || c == b || !und(a, c) || !dir(c, b)) continue;
                    for (size_t d = c + 1; d < N && !fire; ++d)
                        fire = d != a && d != b && und(a, d) && dir(d, b) && !adj(c, d);
                }
                if (fire) {
                    m[b * N + a] = 0;
                    changed = true;
                }
            }
    }
}

bool pdag_to_dag(int32_t n, const uint8_t* pdag, std::vector<std::vector<int32_t>>& parents) {
    const size_t N = size_t(n);
    std::vector<uint8_t> m(pdag, pdag + N * N);
    for (size_t v = 0; v < N; ++v) m[v * N + v] = 0;
    std::vector<uint8_t> gone(N, 0);
    parents.assign(N, {});
    for (size_t a = 0; a < N; ++a)   // the directed edges stay
        for (size_t b = 0; b < N; ++b)
            if (m[a * N + b] && !m[b * N + a]) parents[b].push_back(int32_t(a));
    for (size_t left = N; left > 0; --left) {
        size_t pick = N;
        for (size_t x = 0; x < N && pick == N; ++x) {
            if (gone[x]) continue;
            bool ok = true;
            for (size_t y = 0; y < N && ok; ++y)   // a sink among what remains
                ok = gone[y] || !(m[x * N + y] && !m[y * N + x]);
            for (size_t y = 0; y < N && ok; ++y) {
                if (gone[y] || !(m[x * N + y] && m[y * N + x])) continue;   // y: an undirected neighbour
                for (size_t w = 0; w < N && ok; ++w)
                    if (w != y && !gone[w] && (m[x * N + w] || m[w * N + x])) ok = m[y * N + w] || m[w * N + y];
            }
            if (ok) pick = x;
        }
        if (pick == N) return false;
        for (size_t y = 0; y < N; ++y)
            if (!gone[y] && m[pick * N + y] && m[y * N + pick]) parents[pick].push_back(int32_t(y));
        gone[pick] = 1;
    }
    for (auto& p : parents) std::sort(p.begin(), p.end());
    return true;
}

}  // namespace bnmi
