// Split-K heavy rows (SURVEY.md §5 "long rows"; the reference loops such a row inside one
// thread, WALSEngine.cpp:277-287): rows with more than QMFX_HEAVY_MIN signals are cut into
// QMFX_SEG_LEN-signal segments.  Pass 1: the direct kernel in mode 1, one wave per segment,
// writes the segment's partial Gram tiles, rhs, Σc and negative-weight flag.  Pass 2:
// heavy_reduce_kernel sums a row's segments in fixed order in fp64 with G + λI.  Pass 3: the
// direct kernel in mode 2 solves the row from that image (no signals).  At k > 128 passes 1 and
// 3 are the multi-wave row kernel's modes (wals_big.hip) and pass 2 is heavy_reduce_big_kernel.
#include "direct.h"

namespace qmfx {

// ---------------------------------------------------------------------------------------
// Split-K heavy rows, second pass: one wave per (heavy row h, tile t).  Tile t < NTT: the
// row's segments' partial tiles summed in fp64 in segment order, plus G + λI (the direct
// kernel's tile image), rounded once to T and written over the first segment's tile t
// (only this wave reads that tile, and it reads it first).  t = NTT: the rhs, Σc and the
// negative-weight flag.  Deterministic: the segment order is fixed.
// ---------------------------------------------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(64) void heavy_reduce_kernel(T* part, T* partb, double* partc,
                                                          const int64_t* hseg, int64_t h0,
                                                          const T* Gimg) {
  constexpr int KP = 16 * NT;
  constexpr int NTT = NT * (NT + 1) / 2;
  const int lane = threadIdx.x;
  const int t = blockIdx.y;
  const int64_t h = h0 + blockIdx.x;
  const int64_t s0 = hseg[h], s1 = hseg[h + 1];
  if (t < NTT) {
    const int64_t off = (int64_t)(t * 64 + lane) * 4;
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (double)Gimg[off + r];
    for (int64_t s = s0; s < s1; ++s) {
      const T* p = part + s * (NTT * 256) + off;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += (double)p[r];
    }
    T* o = part + s0 * (NTT * 256) + off;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (T)v[r];
  } else {
    for (int j = lane; j < KP; j += 64) {
      double b = 0.0;
      for (int64_t s = s0; s < s1; ++s) b += (double)partb[s * KP + j];
      partb[s0 * KP + j] = (T)b;
    }
    if (lane == 0) {
      double c = 0.0, f = 0.0;
      for (int64_t s = s0; s < s1; ++s) {
        c += partc[2 * s];
        f = fmax(f, partc[2 * s + 1]);
      }
      partc[2 * s0] = c;
      partc[2 * s0 + 1] = f;
    }
  }
}

// The multi-wave tilings' (wals_big.hip) second pass, with the tile count at run time.
// G + λI (padding diagonal 1) as the big kernel's tile image [tile][lane][4] (gimg_kernel's
// twin, wals.hip; no column permutation: the big kernel's tiles are canonical)
template <typename T>
__global__ void gimg_big_kernel(const T* G, int nt, int k, double lambda, T* img) {
  using M = Mfma<T>;
  const int KP = 16 * nt, NTT = nt * (nt + 1) / 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= NTT * 256) return;
  const int r = idx & 3, lane = (idx >> 2) & 63, t = idx >> 8;
  int I = 0;
  while (tile_index(I + 1, 0) <= t) ++I;
  const int J = t - tile_index(I, 0);
  const int i = 16 * I + M::crow(lane, r), j = 16 * J + (lane & 15);
  double g = (double)G[(int64_t)i * KP + j];
  if (i == j) g += (i < k) ? lambda : 1.0;
  img[idx] = (T)g;
}

// heavy_reduce_kernel's contract: one workgroup of 256 threads per (heavy row, tile) sums the
// row's segments in segment order in fp64 with G + λI, rounds once and writes over the first
// segment's slot; tile index NTT takes the rhs, Σc and the flag.
template <typename T>
__global__ __launch_bounds__(256) void heavy_reduce_big_kernel(T* part, T* partb, double* partc,
                                                               const int64_t* hseg, int64_t h0,
                                                               const T* Gimg, int nt) {
  const int KP = 16 * nt, NTT = nt * (nt + 1) / 2;
  const int t = blockIdx.y;
  const int64_t h = h0 + blockIdx.x;
  const int64_t s0 = hseg[h], s1 = hseg[h + 1];
  const int tid = threadIdx.x;
  if (t < NTT) {
    const int64_t off = (int64_t)t * 256 + tid;
    double v = (double)Gimg[off];
    for (int64_t s = s0; s < s1; ++s) v += (double)part[s * ((int64_t)NTT * 256) + off];
    part[s0 * ((int64_t)NTT * 256) + off] = (T)v;
  } else {
    for (int j = tid; j < KP; j += 256) {
      double b = 0.0;
      for (int64_t s = s0; s < s1; ++s) b += (double)partb[s * KP + j];
      partb[s0 * KP + j] = (T)b;
    }
    if (tid == 0) {
      double c = 0.0, f = 0.0;
      for (int64_t s = s0; s < s1; ++s) {
        c += partc[2 * s];
        f = fmax(f, partc[2 * s + 1]);
      }
      partc[2 * s0] = c;
      partc[2 * s0 + 1] = f;
    }
  }
}

#ifndef QMFX_KERNELS_ONLY
template <typename T>
static hipError_t heavy_reduce_big(T* part, T* partb, double* partc, const int64_t* hseg,
                                   int64_t h0, int64_t nh, const T* G, T* Gimg, int nt, int k,
                                   double lambda, hipStream_t s) {
  const int NTT = nt * (nt + 1) / 2;
  hipLaunchKernelGGL((gimg_big_kernel<T>), dim3(NTT), dim3(256), 0, s, G, nt, k, lambda, Gimg);
  for (int64_t done = 0; done < nh; done += 65535) {
    const int64_t cnt = nh - done < 65535 ? nh - done : 65535;
    hipLaunchKernelGGL((heavy_reduce_big_kernel<T>), dim3((unsigned)cnt, NTT + 1), dim3(256), 0,
                       s, part, partb, partc, hseg, h0 + done, (const T*)Gimg, nt);
  }
  return hipGetLastError();
}
hipError_t launch_heavy_reduce_big(float* part, float* partb, double* partc, const int64_t* hseg,
                                   int64_t h0, int64_t nh, const float* G, float* Gimg, int nt,
                                   int k, double lambda, hipStream_t s) {
  return heavy_reduce_big(part, partb, partc, hseg, h0, nh, G, Gimg, nt, k, lambda, s);
}
hipError_t launch_heavy_reduce_big(double* part, double* partb, double* partc, const int64_t* hseg,
                                   int64_t h0, int64_t nh, const double* G, double* Gimg, int nt,
                                   int k, double lambda, hipStream_t s) {
  return heavy_reduce_big(part, partb, partc, hseg, h0, nh, G, Gimg, nt, k, lambda, s);
}

template <typename T, int NT>
static hipError_t launch_heavy_reduce_nt(T* part, T* partb, double* partc, const int64_t* hseg,
                                         int64_t h0, int64_t nh, const T* Gimg, hipStream_t s) {
  constexpr int NTT = NT * (NT + 1) / 2;
  for (int64_t done = 0; done < nh; done += 65535) {
    const int64_t cnt = nh - done < 65535 ? nh - done : 65535;
    hipLaunchKernelGGL((heavy_reduce_kernel<T, NT>), dim3((unsigned)cnt, NTT + 1), dim3(64), 0, s,
                       part, partb, partc, hseg, h0 + done, Gimg);
  }
  return hipGetLastError();
}
hipError_t launch_heavy_reduce(float* part, float* partb, double* partc, const int64_t* hseg,
                               int64_t h0, int64_t nh, const float* Gimg, int nt, hipStream_t s) {
  return dispatch_nt<1, 8>(nt, [&](auto N) {
    return launch_heavy_reduce_nt<float, decltype(N)::value>(part, partb, partc, hseg, h0, nh,
                                                             Gimg, s);
  });
}
hipError_t launch_heavy_reduce(double* part, double* partb, double* partc, const int64_t* hseg,
                               int64_t h0, int64_t nh, const double* Gimg, int nt, hipStream_t s) {
  return dispatch_nt<1, 8>(nt, [&](auto N) {
    return launch_heavy_reduce_nt<double, decltype(N)::value>(part, partb, partc, hseg, h0, nh,
                                                              Gimg, s);
  });
}

template <typename T>
static hipError_t heavy_seg(const SolveArgs<T>& a, int nt, hipStream_t s) {
  return dispatch_nt<1, 8>(nt, [&](auto N) {
    if (a.seg_mode == 1) return launch_direct_mode<T, decltype(N)::value, 1>(a, s);
    if (a.seg_mode == 2) return launch_direct_mode<T, decltype(N)::value, 2>(a, s);
    return hipErrorInvalidValue;
  });
}
hipError_t launch_wals_heavy(const SolveArgs<float>& a, int nt, hipStream_t s) {
  return heavy_seg(a, nt, s);
}
hipError_t launch_wals_heavy(const SolveArgs<double>& a, int nt, hipStream_t s) {
  return heavy_seg(a, nt, s);
}
#endif  // QMFX_KERNELS_ONLY

}  // namespace qmfx
