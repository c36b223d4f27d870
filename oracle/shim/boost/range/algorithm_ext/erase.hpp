// oracle/shim/boost/range/algorithm_ext/erase.hpp -- TEST INFRASTRUCTURE, this project's own text.
//
// The one name the reference takes from Boost.Range (k2_algorithm::operator()): boost::remove_erase_if(container, pred)
// removes every element the predicate accepts, keeps the others in their order, and returns the container.
#ifndef BN_ORACLE_SHIM_BOOST_RANGE_ALGORITHM_EXT_ERASE_HPP
#define BN_ORACLE_SHIM_BOOST_RANGE_ALGORITHM_EXT_ERASE_HPP

#include <algorithm>

namespace boost {

template<class Container, class Predicate>
Container& remove_erase_if(Container& on, Predicate pred)
{
    on.erase(std::remove_if(on.begin(), on.end(), pred), on.end());
    return on;
}

} // namespace boost

#endif
