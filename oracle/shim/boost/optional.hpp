// oracle/shim/boost/optional.hpp -- TEST INFRASTRUCTURE, this project's own text.
//
// The reference's sampler.hpp includes <boost/optional.hpp> and never names anything from it.  This stand-in lets that
// include resolve where Boost is not installed; it declares the class template so that a use would fail at compile time
// instead of silently meaning something else.
#ifndef BN_ORACLE_SHIM_BOOST_OPTIONAL_HPP
#define BN_ORACLE_SHIM_BOOST_OPTIONAL_HPP

namespace boost {

template<class T> class optional;   // declared, never defined: nothing the oracle compiles may instantiate it

} // namespace boost

#endif
