// One row's WALS system in fp64, assembled by a 256-thread workgroup: shared by the pivoted
// re-solve (fallback.hip) and the explanation kernel (explain.hip), so both form exactly the
// A that qmfx_wals_row_system returns.
#pragma once
#include "common.h"
#include "kernels.h"

namespace qmfx {

constexpr int FB_THREADS = 256;
constexpr int FB_CHUNK = 16;

// Builds A (KP×KP; padding diagonal 1), b and Σc of the signals [beg, end) into A and b.
// PACKED = false: A row-major with row stride KP.  PACKED = true: only the lower triangle,
// element (i, j ≤ i) at A[i(i+1)/2 + j] (the same sums in the same order).  ys: the staging
// rows, LD ≥ KP doubles each.
template <typename T, int LD, bool PACKED>
__device__ void build_system(const FallbackArgs<T>& a, int64_t beg, int64_t end, double* A,
                             double* b, double& csum, double (*ys)[LD], double* ws,
                             double* cs, int tid) {
  const int KP = a.kp, k = a.k;
  for (int idx = tid; idx < KP * KP; idx += FB_THREADS) {
    const int i = idx / KP, j = idx % KP;
    if (PACKED && j > i) continue;
    double v = (i < k && j < k) ? (double)a.G[idx] : 0.0;
    if (i == j) v += i < k ? (double)a.lambda : 1.0;
    A[PACKED ? i * (i + 1) / 2 + j : idx] = v;
  }
  for (int i = tid; i < KP; i += FB_THREADS) b[i] = 0.0;
  double cacc = 0.0;
  __syncthreads();
  for (int64_t base = beg; base < end; base += FB_CHUNK) {
    const int m = (int)(end - base < FB_CHUNK ? end - base : FB_CHUNK);
    for (int idx = tid; idx < FB_CHUNK * KP; idx += FB_THREADS) {
      const int e = idx / KP, j = idx % KP;
      ys[e][j] = (e < m && j < k) ? (double)a.Y[(size_t)(uint32_t)a.col[base + e] * KP + j] : 0.0;
    }
    if (tid < FB_CHUNK) {
      const double v = tid < m ? (double)a.val[base + tid] : 0.0;
      ws[tid] = tid < m ? (double)a.alpha * v : 0.0;
      cs[tid] = tid < m ? 1.0 + (double)a.alpha * v : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < KP * KP; idx += FB_THREADS) {
      const int i = idx / KP, j = idx % KP;
      if (PACKED && j > i) continue;
      double s = 0.0;
#pragma unroll
      for (int e = 0; e < FB_CHUNK; ++e) s += ws[e] * ys[e][i] * ys[e][j];
      A[PACKED ? i * (i + 1) / 2 + j : idx] += s;
    }
    for (int i = tid; i < KP; i += FB_THREADS) {
      double s = 0.0;
#pragma unroll
      for (int e = 0; e < FB_CHUNK; ++e) s += cs[e] * ys[e][i];
      b[i] += s;
    }
    if (tid == 0)
      for (int e = 0; e < m; ++e) cacc += cs[e];
    __syncthreads();
  }
  csum = cacc;  // valid on thread 0
}

}  // namespace qmfx
