// A run-time int as a template argument, for a LISTED set of values: the list is part of the call, so what a launch
// instantiates can be read off it.
#ifndef WXA_DISPATCH_HPP_
#define WXA_DISPATCH_HPP_

#include <type_traits>
#include <utility>

namespace wxa {

// f(std::integral_constant<int, V>) for the listed V that equals v; the last one listed takes every other value (the
// entry points have validated v)
template <int First, int... Rest, class F>
auto with_int(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, First>{});
    else if (v == First) return f(std::integral_constant<int, First>{});
    else return with_int<Rest...>(v, std::forward<F>(f));
}

}  // namespace wxa
#endif
