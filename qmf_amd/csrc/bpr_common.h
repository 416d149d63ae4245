// What the BPR kernels share (bpr.hip: the Hogwild epoch; bpr_foldin.hip: new users' rows
// against frozen items): a factor row across the lanes of a wave64, the step's wave-wide sum
// and loss derivative, and the counter-based negative sampler.
#pragma once
#include "common.h"
#include "rowsolve.h"

namespace qmfx {

// lane l holds factor elements l, l + 64, …, l + 64·(E − 1) of a row (KP ≤ 64·E)
template <typename T, int E>
struct Row {
  T v[E];
};

// x̂ of one (u, p, n) step summed over the wave: 16-lane DPP row sums, then the four rows'
// sums in a fixed order (no LDS round trips; the value is wave-uniform)
template <typename T>
__device__ __forceinline__ T wave_total(T v) {
  v = row16_sum(v);
  return (readlane(v, 0) + readlane(v, 16)) + (readlane(v, 32) + readlane(v, 48));
}
// lossDerivative (BPREngine.cpp:240-244): 1 / (1 + e^x̂).  fp32: the hardware exp2 and
// reciprocal (≤ 1 ulp each); fp64: exact library calls
__device__ __forceinline__ float neg_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.f + __expf(x));
}
__device__ __forceinline__ double neg_sigmoid(double x) { return 1.0 / (1.0 + exp(x)); }

// murmur3 32-bit finaliser (a bijection of uint32)
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  return x ^ (x >> 16);
}

// Negative sampling (sampleRandomNegative, BPREngine-inl.h:48-60, which draws from
// mt19937): counter-based instead, so every draw is reproducible for a given seed.  Positive
// slot s has the 64-bit key mix64(seed_key ^ s) (one splitmix64 per positive); draw j,
// attempt t of it is fmix32(fold(key) + (4099·j + t)·φ) scaled to [0, nitems) — a bijection
// of the counter, all in 32-bit scalar arithmetic.
__device__ __forceinline__ uint32_t draw_hash(uint32_t fk, uint32_t ctr) {
  return fmix32(fk + ctr * 0x9e3779b9u);
}
__device__ __forceinline__ int64_t draw_candidate(uint32_t fk, uint32_t ctr, uint32_t nitems) {
  return (int64_t)(((uint64_t)draw_hash(fk, ctr) * nitems) >> 32);
}

// Rejection-samples a negative for user u: uniform in [0, nitems) and not in the user's
// positive set (sorted list urowptr/uitems).  fk = the positive's folded key, ctr0 = 4099·j.
__device__ __forceinline__ int64_t sample_negative(const int32_t* items, int64_t cnt,
                                                   uint32_t nitems, uint32_t fk, uint32_t ctr0,
                                                   int lane) {
  for (uint32_t attempt = 0;; ++attempt) {
    const int64_t cand = draw_candidate(fk, ctr0 + attempt, nitems);
    bool hit = false;
    for (int64_t base = 0; base < cnt; base += 64) {
      const int64_t j = base + lane;
      const bool m = j < cnt && items[j] == cand;
      if (__any(m)) {
        hit = true;
        break;
      }
    }
    if (!hit || attempt >= 4096) return cand;
  }
}

// Draws the negative for (slot, j) against the user's positives: the first 64 are staged in
// `mine` (one per lane); longer lists are scanned from memory.
template <typename A>
__device__ __forceinline__ int64_t draw_negative_t(const A& a, const int32_t* items, int64_t cnt,
                                                   int32_t mine, uint32_t fk, uint32_t ctr0,
                                                   int lane) {
  const uint32_t ni = (uint32_t)a.nitems;
  if (cnt > 64) return sample_negative(items, cnt, ni, fk, ctr0, lane);
  for (uint32_t attempt = 0;; ++attempt) {
    const int64_t cand = draw_candidate(fk, ctr0 + attempt, ni);
    if (!__any(mine == (int32_t)cand) || attempt >= 4096) return cand;
  }
}

// E = ceil(KP / 64) as a template argument
#define QMFX_E_SWITCH(KP, CALL)          \
  switch ((KP + 63) / 64) {              \
    case 1: return CALL(1);              \
    case 2: return CALL(2);              \
    case 3: return CALL(3);              \
    case 4: return CALL(4);              \
    default: return hipErrorInvalidValue; \
  }

}  // namespace qmfx
