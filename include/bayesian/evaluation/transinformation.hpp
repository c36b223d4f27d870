// bayesian/evaluation/transinformation.hpp -- drop-in for the reference's bn::evaluation::entropy and
// bn::evaluation::mutual_information (bayesian/evaluation/transinformation.hpp:10-84), computed on the
// MI355X through bn_info_* (include/bn_mi355x.h).  C++14.
//
// Same functors, same five overloads: entropy(sampling, variables), entropy(sampling, variable),
// mutual_information(sampling, x, y), the template (sampling, x, x_ent, y, y_ent) and the template
// (x_ent, y_ent, xy_ent).  Only the requested variables' columns of sampling.table() are marshalled; a
// variable's arity is its selectable_num; a pattern lacking a requested variable throws std::out_of_range
// (condition_t::at, :23).  An empty sampler gives 0.0 without touching the GPU.  An error of the C ABI
// throws std::runtime_error.
//
// Differences from the reference:
//   - the reference's header does not compile (entropy::operator() calls lower_bound / key_comp on an
//     unordered_map, :26-27); this is its first working form;
//   - a listed pattern with occurrence 0 contributes nothing (the reference would add 0 * log2(0) = NaN);
//   - a set's joint key is limited to 64 bits: the product of the arities of the distinct variables of
//     arity >= 2 must be <= 2^64.
// Not in the reference (labelled so below): information_table, a set of columns kept on the device for
// repeated queries, and mutual_information_matrix.
#ifndef BNI_EVALUATION_TRANSINFORMATION_HPP
#define BNI_EVALUATION_TRANSINFORMATION_HPP

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include <bayesian/graph.hpp>
#include <bayesian/sampler.hpp>
#include <bn_mi355x.h>

namespace bn {
namespace evaluation {

// NOT IN THE REFERENCE: the columns `variables` of a sampler's table, uploaded once.  Queries name
// variables of that list.
class information_table {
public:
    struct matrix {
        std::size_t m = 0;
        std::vector<double> h;      // [m]
        std::vector<double> hxy;    // [m][m], symmetric, diagonal h
        std::vector<double> mi;     // [m][m] = h[x] + h[y] - hxy[x][y]
    };

    // rows_out (may be null): the distinct patterns in the order they were uploaded (row i of the device table)
    information_table(sampler const& sampling, std::vector<vertex_type> const& variables, int device = BN_DEVICE_CURRENT,
                      std::vector<condition_t>* rows_out = nullptr)
        : vars_(unique(variables))
    {
        if(sampling.sampling_size() == 0) return;
        auto const table = sampling.table();
        std::vector<std::uint8_t> patterns;
        std::vector<std::uint64_t> counts;
        std::vector<std::int32_t> k;
        patterns.reserve(table.size() * vars_.size());
        counts.reserve(table.size());
        for(auto const& v : vars_) k.push_back(static_cast<std::int32_t>(v->selectable_num));
        for(auto const& sample : table)
        {
            for(auto const& v : vars_) patterns.push_back(static_cast<std::uint8_t>(sample.first.at(v)));
            counts.push_back(static_cast<std::uint64_t>(sample.second));
            if(rows_out) rows_out->push_back(sample.first);
        }
        mi355x::engine_handle::check(bn_info_create(static_cast<std::int64_t>(counts.size()), static_cast<std::int32_t>(vars_.size()),
                                                    patterns.data(), counts.data(), k.data(), device, &table_));
    }
    ~information_table() { bn_info_destroy(table_); }
    information_table(information_table const&) = delete;
    information_table& operator=(information_table const&) = delete;

    std::vector<vertex_type> const& variables() const { return vars_; }
    // the C handle (null for an empty sampler): what bn_score_* of include/bn_mi355x.h take
    bn_info_table* handle() const { return table_; }

    double entropy(std::vector<vertex_type> const& variables) const
    {
        if(!table_) return 0.0;
        std::vector<std::int32_t> cols;
        for(auto const& v : variables) cols.push_back(column(v));
        double h = 0.0;
        mi355x::engine_handle::check(bn_info_entropy(table_, static_cast<std::int32_t>(cols.size()), cols.data(), 0, &h));
        return h;
    }
    double entropy(vertex_type const& variable) const { return entropy(std::vector<vertex_type>{variable}); }

    // every pair of the table's variables at once (one all-pairs kernel)
    matrix pair_entropies() const
    {
        matrix out;
        out.m = vars_.size();
        out.h.assign(out.m, 0.0);
        out.hxy.assign(out.m * out.m, 0.0);
        out.mi.assign(out.m * out.m, 0.0);
        if(table_ && out.m)
            mi355x::engine_handle::check(bn_info_pair_entropies(table_, static_cast<std::int32_t>(out.m), nullptr, out.h.data(),
                                                                out.hxy.data(), out.mi.data()));
        return out;
    }

private:
    static std::vector<vertex_type> unique(std::vector<vertex_type> const& v)
    {
        std::vector<vertex_type> out;
        for(auto const& x : v)
            if(std::find(out.begin(), out.end(), x) == out.end()) out.push_back(x);
        return out;
    }
    std::int32_t column(vertex_type const& v) const
    {
        auto const it = std::find(vars_.begin(), vars_.end(), v);
        if(it == vars_.end()) throw std::out_of_range("bn::evaluation::information_table: variable not in the table");
        return static_cast<std::int32_t>(it - vars_.begin());
    }

    std::vector<vertex_type> vars_;
    bn_info_table* table_ = nullptr;
};

struct entropy {
    // joint entropy of `variables` in the samples (transinformation.hpp:14-40)
    double operator() (sampler const& sampling, std::vector<vertex_type> const& variables) const
    {
        if(sampling.sampling_size() == 0) return 0.0;
        return information_table(sampling, variables).entropy(variables);
    }

    double operator() (sampler const& sampling, vertex_type const& variable) const
    {
        std::vector<vertex_type> variables = {variable};
        return (*this)(sampling, variables);
    }
};

struct mutual_information {
    // (transinformation.hpp:55-61): H(x) + H(y) - H(x, y), one table upload for the three entropies
    double operator() (sampler const& sampling, vertex_type const& x, vertex_type const& y) const
    {
        if(sampling.sampling_size() == 0) return 0.0;
        information_table const t(sampling, {x, y});
        return t.entropy(x) + t.entropy(y) - t.entropy({x, y});
    }

    // (:67-72) the entropies of x and y already known
    template<class T>
    double operator() (sampler const& sampling, vertex_type const& x, T const x_ent, vertex_type const& y, T const y_ent) const
    {
        entropy ent;
        return x_ent + y_ent - ent(sampling, {x, y});
    }

    // (:77-81)
    template<class T>
    double operator() (T const x_ent, T const y_ent, T const xy_ent) const
    {
        return x_ent + y_ent - xy_ent;
    }
};

// NOT IN THE REFERENCE: h, hxy and mi of every pair of `variables` (distinct, in first-appearance order)
inline information_table::matrix mutual_information_matrix(sampler const& sampling, std::vector<vertex_type> const& variables)
{
    return information_table(sampling, variables).pair_entropies();
}

} // namespace evaluation
} // namespace bn

#endif // BNI_EVALUATION_TRANSINFORMATION_HPP
