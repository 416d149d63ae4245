// The fp64 inverse Cholesky factor of G + λI, the operand of the whitening GEMMs
// (whiten.hip) that put the whitened row kernels (woodbury.hip) in a basis where G + λI = I.
#include "kernels.h"
#include "ntswitch.h"

namespace qmfx {

// ---------------------------------------------------------------------------------------
// M = G + λI (padding: 1) → L (Cholesky, fp64, in LDS) → Linv = L⁻¹ written in T.
// One 256-thread workgroup; run once per half when whitened rows exist.
// ---------------------------------------------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(256) void chol_inv_kernel(const T* G, int k, double lambda,
                                                       T* Linv, int32_t* status) {
  constexpr int KP = 16 * NT;
  constexpr int LD = KP + 1;
  __shared__ double A[KP * LD];
  __shared__ double dinv[KP];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < KP * KP; idx += 256) {
    const int i = idx / KP, j = idx % KP;
    double v = (double)G[idx];
    if (i == j) v += i < k ? lambda : 1.0;
    A[i * LD + j] = v;
  }
  __syncthreads();
  for (int j = 0; j < KP; ++j) {
    if (tid == 0) {
      const double d = A[j * LD + j];
      if (!(d > 0.0)) *status = 1;
      const double l = sqrt(d > 0.0 ? d : 1.0);
      A[j * LD + j] = l;
      dinv[j] = 1.0 / l;
    }
    __syncthreads();
    for (int i = j + 1 + tid; i < KP; i += 256) A[i * LD + j] *= dinv[j];
    __syncthreads();
    const int m = KP - j - 1;  // trailing size
    for (int idx = tid; idx < m * m; idx += 256) {
      const int ii = j + 1 + idx / m, mm = j + 1 + idx % m;
      if (mm <= ii) A[ii * LD + mm] -= A[ii * LD + j] * A[mm * LD + j];
    }
    __syncthreads();
  }
  // Linv column c (thread c): Linv[c][c] = 1/L[c][c];
  // Linv[i][c] = −(Σ_{m=c}^{i−1} L[i][m] Linv[m][c]) / L[i][i], kept in A's upper triangle
  // at A[c][i] (row c is private to thread c)
  if (tid < KP) {
    const int c = tid;
    for (int i = c + 1; i < KP; ++i) {
      double s = A[i * LD + c] * dinv[c];
      for (int m = c + 1; m < i; ++m) s += A[i * LD + m] * A[c * LD + m];
      A[c * LD + i] = -s * dinv[i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < KP * KP; idx += 256) {
    const int i = idx / KP, c = idx % KP;
    double v = 0.0;
    if (i == c) v = dinv[c];
    else if (i > c) v = A[c * LD + i];
    Linv[idx] = (T)v;
  }
}

// The same factorization for KP > 128 (the fp64 matrix exceeds LDS): one 1024-thread
// workgroup on a global fp64 scratch of KP·(KP+1) doubles (L2-resident; __syncthreads
// orders the block's global accesses).  Once per half; ≈ms at KP = 256.
template <typename T, int NT>
__global__ __launch_bounds__(1024) void chol_inv_global_kernel(const T* G, int k, double lambda,
                                                               T* Linv, int32_t* status,
                                                               double* A) {
  constexpr int KP = 16 * NT;
  constexpr int LD = KP + 1;
  static_assert(4 * KP <= 1024, "the inverse gives each of the KP columns 4 of the 1024 threads");
  __shared__ double dinv[KP];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < KP * KP; idx += 1024) {
    const int i = idx / KP, j = idx % KP;
    double v = (double)G[idx];
    if (i == j) v += i < k ? lambda : 1.0;
    A[i * LD + j] = v;
  }
  __syncthreads();
  for (int j = 0; j < KP; ++j) {
    if (tid == 0) {
      const double d = A[j * LD + j];
      if (!(d > 0.0)) *status = 1;
      const double l = sqrt(d > 0.0 ? d : 1.0);
      A[j * LD + j] = l;
      dinv[j] = 1.0 / l;
    }
    __syncthreads();
    for (int i = j + 1 + tid; i < KP; i += 1024) A[i * LD + j] *= dinv[j];
    __syncthreads();
    const int m = KP - j - 1;
    for (int idx = tid; idx < m * m; idx += 1024) {
      const int ii = j + 1 + idx / m, mm = j + 1 + idx % m;
      if (mm <= ii) A[ii * LD + mm] -= A[ii * LD + j] * A[mm * LD + j];
    }
    __syncthreads();
  }
  // L⁻¹ column c by forward substitution on four threads (lanes 4c .. 4c + 3 of one wave):
  // thread q sums the terms mm ≡ q (mod 4), two shuffles combine them, and entry i is stored
  // by the thread that will read it again (q = i mod 4), so each thread only re-reads its own
  // writes.  One thread per column left the k = 256 launch at 6.2 ms, the column chains
  // (up to 32K dependent-address FMAs) being the whole of it.
  {
    const int c = tid >> 2, q = tid & 3;
    if (c < KP) {
      for (int i = c + 1; i < KP; ++i) {
        double sm = q == 0 ? A[i * LD + c] * dinv[c] : 0.0;
        int mm = c + 1 + ((q - (c + 1)) & 3);
        for (; mm < i; mm += 4) sm += A[i * LD + mm] * A[c * LD + mm];
        sm += __shfl_xor(sm, 1, 64);
        sm += __shfl_xor(sm, 2, 64);
        if ((i & 3) == q) A[c * LD + i] = -sm * dinv[i];
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < KP * KP; idx += 1024) {
    const int i = idx / KP, c = idx % KP;
    double v = 0.0;
    if (i == c) v = dinv[c];
    else if (i > c) v = A[c * LD + i];
    Linv[idx] = (T)v;
  }
}

#ifndef QMFX_KERNELS_ONLY
template <typename T, int NT>
static hipError_t launch_chol_inv_nt(const T* G, int k, double lambda, T* Linv, int32_t* status,
                                     double* scratch, hipStream_t s) {
  if constexpr (NT > 8) {
    if (!scratch) return hipErrorInvalidValue;
    hipLaunchKernelGGL((chol_inv_global_kernel<T, NT>), dim3(1), dim3(1024), 0, s, G, k, lambda,
                       Linv, status, scratch);
    return hipGetLastError();
  } else {
    (void)scratch;
    hipLaunchKernelGGL((chol_inv_kernel<T, NT>), dim3(1), dim3(256), 0, s, G, k, lambda, Linv,
                       status);
    return hipGetLastError();
  }
}

hipError_t launch_chol_inv(const float* G, int nt, int k, double lambda, float* Linv,
                           int32_t* status, double* scratch, hipStream_t s) {
  return dispatch_nt_w(nt, [&](auto N) {
    return launch_chol_inv_nt<float, decltype(N)::value>(G, k, lambda, Linv, status, scratch, s);
  });
}
hipError_t launch_chol_inv(const double* G, int nt, int k, double lambda, double* Linv,
                           int32_t* status, double* scratch, hipStream_t s) {
  return dispatch_nt_w(nt, [&](auto N) {
    return launch_chol_inv_nt<double, decltype(N)::value>(G, k, lambda, Linv, status, scratch, s);
  });
}
#endif  // QMFX_KERNELS_ONLY

}  // namespace qmfx
