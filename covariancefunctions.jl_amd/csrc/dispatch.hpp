// dispatch.hpp — a runtime value becomes a template argument of a launch: ONE generic lambda per launch instead of a ladder per value.  For the host
// drivers (through driver.hpp) and for the launchers of the per-family kernel units, which include this and common.hpp, not the drivers' header.
#pragma once
#include <type_traits>
#include <utility>

#include "common.hpp"

namespace covgram {

// f(float{}) or f(double{}): ONE generic lambda for both element types of a launch
template <typename F>
inline decltype(auto) by_dtype(int dtype, F&& f) {
    if (dtype == COVGRAM_F32) return f(float{});
    return f(double{});
}

// f(std::true_type{}) or f(std::false_type{}): the same for a flag that is a template argument of the launch
template <typename F>
inline decltype(auto) by_bool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// The same for a padded dimension (or another small integer) that is a template argument of the launch.  Dims<...> is the call site's list of
// compiled buckets — the set of its kernel instances.  try_dim: f(std::integral_constant<int, D>{}) for the bucket that equals the runtime D;
// false where D is not in the list (the caller has another kernel for those).  by_dim: f returns the launch's status, and a D outside the
// list is refused with the site's own text (`refusal`, one %d).
template <int... Ds> using Dims = std::integer_sequence<int, Ds...>;
template <int... Ds, typename F>
inline bool try_dim(Dims<Ds...>, int D, F&& f) {
    return ((D == Ds && (f(std::integral_constant<int, Ds>{}), true)) || ...);
}
template <int... Ds, typename F>
inline int by_dim(Dims<Ds...> dims, int D, const char* refusal, F&& f) {
    int rc = COVGRAM_EUNSUPPORTED;
    if (!try_dim(dims, D, [&](auto d) { rc = f(d); })) set_error(refusal, D);
    return rc;
}

}  // namespace covgram
