// Runtime values -> template arguments, for the launch helpers that take a plan (gemm_plan.h, gemv_plan.h) and only launch.
#pragma once
#include <type_traits>

namespace teo {

// f(std::integral_constant<bool, b>...) with every runtime flag turned into a compile-time one: the launch helpers' way of picking a
// template instantiation (each call instantiates f for all 2^n combinations of its flags, no more)
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename F>
decltype(auto) with_flags(F&& f) { return f(); }
template <typename F, typename... B>
decltype(auto) with_flags(F&& f, bool b, B... rest) {
    if (b) return with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
    return with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

}  // namespace teo
