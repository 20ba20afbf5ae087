// Run-time (d, q) -> compile-time template dispatch of the passes over the records whose kernels depend on (d, q) alone
// (datalik.hip, datalik_times.hip, events.hip and their host builds under tests/emul/).  A pass is built for
//   1 <= d <= MaxD,  1 <= q <= 5,  d (q + 1) <= MaxState;
// its predicate and its dispatch are both stated through these constants.  Includes no kernel header.
#pragma once
#include <type_traits>
#include <utility>

namespace odef {

template <int MaxD, int MaxState>
constexpr bool has_dq(int d, int q) {
  return d >= 1 && d <= MaxD && q >= 1 && q <= 5 && d * (q + 1) <= MaxState;
}

template <int MaxD, int MaxState, class F, int... I>
inline bool dispatch_dq_seq(int d, int q, F& f, std::integer_sequence<int, I...>) {
  auto one = [&](auto ic) {  // pair number I = 5 (d - 1) + (q - 1)
    constexpr int dd = decltype(ic)::value / 5 + 1, qq = decltype(ic)::value % 5 + 1;
    if constexpr (has_dq<MaxD, MaxState>(dd, qq)) {
      if (d == dd && q == qq) {
        f.template operator()<dd, qq>();
        return true;
      }
    }
    return false;
  };
  return (... || one(std::integral_constant<int, I>{}));
}

// calls f.template operator()<d, q>() when the pass has an instance for (d, q); false: it has none
template <int MaxD, int MaxState, class F>
inline bool dispatch_dq(int d, int q, F&& f) {
  return dispatch_dq_seq<MaxD, MaxState>(d, q, f, std::make_integer_sequence<int, 5 * MaxD>{});
}

}  // namespace odef
