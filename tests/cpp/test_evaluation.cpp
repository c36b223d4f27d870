// tests/cpp/test_evaluation.cpp -- bn::evaluation::entropy / mutual_information (include/bayesian/evaluation/
// transinformation.hpp) over this repository's stand-in data model (-Iinclude -Iinclude/compat), C++14.
// Modes:  (default)  an empty sampler: every overload gives 0.0 without a device
//         --gpu      a random table over 7 variables of mixed arities: the five reference overloads and
//                    mutual_information_matrix against a std::map restatement inside this program
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include <bayesian/evaluation/transinformation.hpp>
#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>

namespace {

int failures = 0;

void expect_close(double got, double want, char const* what)
{
    if(!(std::fabs(got - want) <= 1e-12 * std::max(1.0, std::fabs(want))))
    {
        std::printf("MISMATCH %s: got %.17g want %.17g\n", what, got, want);
        ++failures;
    }
}

// the reference's formula over an ordered map of the variables' joint states
double restated_entropy(std::unordered_map<bn::condition_t, std::size_t> const& table, std::vector<bn::vertex_type> const& vars,
                        std::size_t total)
{
    std::map<std::vector<int>, std::size_t> cells;
    for(auto const& sample : table)
    {
        std::vector<int> key;
        for(auto const& v : vars) key.push_back(sample.first.at(v));
        cells[key] += sample.second;
    }
    double h = 0.0;
    for(auto const& c : cells)
    {
        if(c.second == 0) continue;
        double const p = static_cast<double>(c.second) / static_cast<double>(total);
        h -= p * std::log2(p);
    }
    return h;
}

} // namespace

int main(int argc, char** argv)
{
    bool const gpu = argc > 1 && std::strcmp(argv[1], "--gpu") == 0;
    bn::graph_t g;
    std::vector<bn::vertex_type> v;
    int const arity[] = {2, 3, 4, 1, 17, 40, 5};
    for(int i = 0; i < 7; ++i)
    {
        auto x = g.add_vertex();
        x->id = i + 1;
        x->selectable_num = static_cast<std::size_t>(arity[i]);
        v.push_back(x);
    }
    bn::evaluation::entropy const ent;
    bn::evaluation::mutual_information const mi;

    if(!gpu)
    {
        bn::sampler const empty;
        if(ent(empty, v) != 0.0 || ent(empty, v[0]) != 0.0 || mi(empty, v[0], v[1]) != 0.0 ||
           mi(empty, v[0], 0.5, v[1], 0.25) != 0.75 || mi(1.0, 2.0, 2.5) != 0.5 ||
           bn::evaluation::mutual_information_matrix(empty, v).hxy != std::vector<double>(49, 0.0))
        {
            std::printf("empty sampler: not 0.0\n");
            return 1;
        }
        std::printf("evaluation empty ok\n");
        return 0;
    }

    std::mt19937 rng(12345);
    std::unordered_map<bn::condition_t, std::size_t> table;
    std::size_t total = 0;
    for(int s = 0; s < 3000; ++s)
    {
        bn::condition_t pattern;
        for(int i = 0; i < 7; ++i) pattern[v[i]] = static_cast<int>(rng() % static_cast<unsigned>(arity[i]));
        std::size_t const c = 1 + rng() % 50;
        table[pattern] += c;
        total += c;
    }
    bn::sampler sampling;
    sampling.load_sample(table);

    expect_close(ent(sampling, v[4]), restated_entropy(table, {v[4]}, total), "entropy(sampling, variable)");
    expect_close(ent(sampling, {v[0], v[2], v[5]}), restated_entropy(table, {v[0], v[2], v[5]}, total), "entropy(sampling, variables)");
    expect_close(ent(sampling, {v[1], v[1]}), restated_entropy(table, {v[1]}, total), "entropy with a duplicate");
    expect_close(ent(sampling, v[3]), 0.0, "entropy of an arity-1 variable");
    double const hx = restated_entropy(table, {v[1]}, total), hy = restated_entropy(table, {v[5]}, total);
    double const hxy = restated_entropy(table, {v[1], v[5]}, total);
    expect_close(mi(sampling, v[1], v[5]), hx + hy - hxy, "mutual_information(sampling, x, y)");
    expect_close(mi(sampling, v[1], hx, v[5], hy), hx + hy - hxy, "mutual_information(sampling, x, x_ent, y, y_ent)");
    if(mi(hx, hy, hxy) != hx + hy - hxy) { std::printf("MISMATCH three-entropy overload\n"); ++failures; }
    expect_close(mi(sampling, v[2], v[2]), restated_entropy(table, {v[2]}, total), "MI(x, x) = H(x)");

    auto const m = bn::evaluation::mutual_information_matrix(sampling, v);
    bn::evaluation::information_table const t(sampling, v);
    for(std::size_t x = 0; x < 7; ++x)
        for(std::size_t y = 0; y < 7; ++y)
        {
            double const want = restated_entropy(table, {v[x], v[y]}, total);
            expect_close(m.hxy[x * 7 + y], want, "matrix hxy");
            if(m.hxy[x * 7 + y] != t.entropy({v[x], v[y]})) { std::printf("MISMATCH matrix vs single call bits\n"); ++failures; }
            if(m.mi[x * 7 + y] != m.h[x] + m.h[y] - m.hxy[x * 7 + y]) { std::printf("MISMATCH matrix mi\n"); ++failures; }
        }
    if(failures) return 1;
    std::printf("evaluation gpu ok\n");
    return 0;
}
