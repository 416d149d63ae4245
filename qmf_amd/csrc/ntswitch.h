// Host-side dispatch of a runtime tile count to the kernel template instances.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

// f(integral_constant<int, nt>) for LO ≤ nt ≤ HI, hipErrorInvalidValue otherwise: only the
// tilings of the range are instantiated (the one-wave kernels: 1..8, the fp64 one-wave YᵀY:
// 1..4; the multi-wave kernels' ranges are in kernels.h)
template <int LO, int HI, typename F>
hipError_t dispatch_nt(int nt, F&& f) {
  if constexpr (LO <= HI) {
    if (nt == LO) return f(std::integral_constant<int, LO>{});
    return dispatch_nt<LO + 1, HI>(nt, f);
  } else {
    return hipErrorInvalidValue;
  }
}

// whitened path: every one-wave tiling plus k = 256 (NT = 16, beside the multi-wave direct
// kernel)
template <typename F>
hipError_t dispatch_nt_w(int nt, F&& f) {
  if (nt == 16) return f(std::integral_constant<int, 16>{});
  return dispatch_nt<1, 8>(nt, f);
}
