// gswt_variant.h -- the one way a launch wrapper picks a kernel instantiation from runtime values (gswt_kernels.hip, gswt_passes.hip).
// Host-only and free of HIP: <type_traits> is all it needs (tools/with_variant_main.cpp compiles it with the host compiler alone).
//
// with_variant(fn, a, b, ...) calls the generic lambda fn with one compile-time constant per selector, in the selectors' order -- a bool
// becomes std::bool_constant, OneOf<V0, .., Vn>{v} the std::integral_constant of the Vi that v equals (the last one when it equals none) --
// so that fn names its kernel as k<A, B, ...>.  fn is instantiated for every combination of the selectors: where the kernel has no such
// form, fn guards the launch with `if constexpr` and the wrapper keeps the combination from arriving.
#pragma once
#include <type_traits>

namespace gswt {

template <int... Vs> struct OneOf { int v; };
template <typename Fn>
static void with_variant(Fn&& fn) { fn(); }
template <typename Fn, int V0, int... Vs, typename... Rest>
static void with_variant(Fn&& fn, OneOf<V0, Vs...> sel, Rest... rest);
template <typename Fn, typename... Rest>
static void with_variant(Fn&& fn, bool sel, Rest... rest)
{
    if (sel) with_variant([&](auto... cs) { fn(std::true_type{}, cs...); }, rest...);
    else with_variant([&](auto... cs) { fn(std::false_type{}, cs...); }, rest...);
}
template <typename Fn, int V0, int... Vs, typename... Rest>
static void with_variant(Fn&& fn, OneOf<V0, Vs...> sel, Rest... rest)
{
    if (sizeof...(Vs) == 0 || sel.v == V0) with_variant([&](auto... cs) { fn(std::integral_constant<int, V0>{}, cs...); }, rest...);
    else if constexpr (sizeof...(Vs) != 0) with_variant(fn, OneOf<Vs...>{sel.v}, rest...);
}

}  // namespace gswt
