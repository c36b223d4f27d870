// oracle/shim/boost/algorithm/string.hpp -- TEST INFRASTRUCTURE, this project's own text.
//
// The one call the reference makes into Boost.StringAlgo (sampler::load_sample):
//     boost::algorithm::split(tokens, line, boost::is_space(), boost::algorithm::token_compress_on);
// with Boost's semantics: the input is cut at every character the predicate accepts; with token_compress_on a run of
// adjacent separators counts as one.  Separators at either end are NOT dropped: a line that starts with a blank gives a
// leading empty token, one that ends with a blank a trailing empty token, and an empty line gives one empty token --
// load_sample reads tokens[0] as the count, so the leading token matters.
#ifndef BN_ORACLE_SHIM_BOOST_ALGORITHM_STRING_HPP
#define BN_ORACLE_SHIM_BOOST_ALGORITHM_STRING_HPP

#include <algorithm>
#include <cctype>
#include <string>

namespace boost {
namespace algorithm {

enum token_compress_mode_type { token_compress_on, token_compress_off };

struct is_space_pred {
    bool operator()(char c) const { return std::isspace(static_cast<unsigned char>(c)) != 0; }
};

inline is_space_pred is_space() { return is_space_pred(); }

template<class Sequence, class Predicate>
Sequence& split(Sequence& result, std::string const& input, Predicate pred, token_compress_mode_type mode = token_compress_off)
{
    Sequence tokens;
    auto it = input.begin();
    auto const end = input.end();
    for(;;)
    {
        auto const stop = std::find_if(it, end, pred);
        tokens.emplace_back(it, stop);
        if(stop == end) break;
        it = stop + 1;
        if(mode == token_compress_on) while(it != end && pred(*it)) ++it;
    }
    result.swap(tokens);
    return result;
}

} // namespace algorithm

using algorithm::is_space;

} // namespace boost

#endif
