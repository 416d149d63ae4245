// Host-side dispatch of a runtime tile count to the kernel template instances.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

// f(integral_constant<int, nt>) for LO ≤ nt ≤ HI, hipErrorInvalidValue otherwise: only the
// tilings of the range are instantiated (the multi-wave kernels' ranges are in kernels.h)
template <int LO, int HI, typename F>
hipError_t dispatch_nt(int nt, F&& f) {
  if constexpr (LO <= HI) {
    if (nt == LO) return f(std::integral_constant<int, LO>{});
    return dispatch_nt<LO + 1, HI>(nt, f);
  } else {
    return hipErrorInvalidValue;
  }
}

#define QMFX_NT_SWITCH(NTV, CALL)         \
  switch (NTV) {                          \
    case 1: return CALL(1);               \
    case 2: return CALL(2);               \
    case 3: return CALL(3);               \
    case 4: return CALL(4);               \
    case 5: return CALL(5);               \
    case 6: return CALL(6);               \
    case 7: return CALL(7);               \
    case 8: return CALL(8);               \
    default: return hipErrorInvalidValue; \
  }
// fp32 whitened path: every one-wave tiling plus k = 256 (NT = 16, beside the multi-wave
// direct kernel)
#define QMFX_NT_SWITCH_W(NTV, CALL)       \
  switch (NTV) {                          \
    case 1: return CALL(1);               \
    case 2: return CALL(2);               \
    case 3: return CALL(3);               \
    case 4: return CALL(4);               \
    case 5: return CALL(5);               \
    case 6: return CALL(6);               \
    case 7: return CALL(7);               \
    case 8: return CALL(8);               \
    case 16: return CALL(16);             \
    default: return hipErrorInvalidValue; \
  }
#define QMFX_NT_SWITCH64(NTV, CALL)       \
  switch (NTV) {                          \
    case 1: return CALL(1);               \
    case 2: return CALL(2);               \
    case 3: return CALL(3);               \
    case 4: return CALL(4);               \
    default: return hipErrorInvalidValue; \
  }

