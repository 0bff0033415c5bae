// A run-time integer as a template argument: with_constant<LO, HI>(v, f) calls the generic lambda f
// with std::integral_constant<int, v> when LO <= v <= HI and returns true; otherwise f is not called
// and the result is false, which the caller reports (an order that is not compiled in).  f is
// instantiated for LO..HI and for nothing else.  Host only.
#pragma once
#include <type_traits>
#include <utility>

namespace cmdg {

template <int LO, int HI, class F>
bool with_constant(int value, F &&f)
{
    if constexpr (LO > HI) {
        return false;
    } else {
        if (value != LO) return with_constant<LO + 1, HI>(value, std::forward<F>(f));
        f(std::integral_constant<int, LO>{});
        return true;
    }
}

}  // namespace cmdg
