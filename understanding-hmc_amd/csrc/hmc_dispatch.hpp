// hmc_dispatch.hpp — run-time values to template arguments, for the launchers' instance choice.
// Nested around one kernel launch; the lambda guards an instance that must not exist with `if constexpr`.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace hmc {

// f(std::true_type{}) or f(std::false_type{})
template <class F>
auto with_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the V among Vs that equals v; hipErrorInvalidValue for none
template <int... Vs, class F>
hipError_t with_value(int v, F&& f) {
  hipError_t e = hipErrorInvalidValue;
  (void)((v == Vs && ((e = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return e;
}

}  // namespace hmc
