// YᵀY for the multi-wave tilings (fp32 k > 128, fp64 k > 64; WALSEngine::computeXtX,
// qmf/wals/WALSEngine.cpp:246-264, as in wals.hip): per-block partials of every lower tile
// (gram_tiles_kernel), then the fixed-order fp64 sum and mirror (gram_reduce_rt_kernel).
#include "big.h"
#include "gram_reduce.h"
#include "ntswitch.h"

namespace qmfx {

// ---- YᵀY for large NT, every tile per workgroup: the block's rows are staged through LDS
// SIG at a time with coalesced 16-B loads, so Y is read from HBM once (a strip per block
// row read it NT times: 42 -> 4 ms per launch at C5), and the waves split the NT(NT+1)/2
// tiles as in the row kernel's staged Gram (big_gram_step, weight 1).
template <typename T, int NT>
__global__ __launch_bounds__((BigCfg<T, NT>::NTHR)) void gram_tiles_kernel(
    const T* Y, int64_t n, int64_t rows_per_block, double* partial) {
  using C = BigCfg<T, NT>;
  using M = Mfma<T>;
  using acc_t = typename M::acc_t;
  using vec_t = T __attribute__((ext_vector_type(C::VEC)));
  constexpr int KP = C::KP, NW = C::NW, TPW = C::TPW, NTT = C::NTT, SIG = C::SIG;
  constexpr int CPR = C::CPR, TRIPS = C::TRIPS;
  __shared__ __attribute__((aligned(16))) T stage[SIG * KP];

  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int cl = lane & 15;
  const int kk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;

  int TI[TPW], TJ[TPW];
  acc_t acc[TPW];
#pragma unroll
  for (int s = 0; s < TPW; ++s) {
    big_tile<C>(wv, s, TI[s], TJ[s]);
    acc[s] = acc_t{0, 0, 0, 0};
  }

  // the next stage's rows are loaded into registers while this stage's MFMAs run (the
  // same rows in the same order: the partials are bit-identical to a load-then-compute loop)
  vec_t nx[TRIPS];
  auto fetch = [&](int64_t e0) {
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int ch = tid + C::NTHR * t;
      const int64_t e = e0 + ch / CPR;
      nx[t] = (ch < SIG * CPR && e < r1)
                  ? *(reinterpret_cast<const vec_t*>(Y + e * KP) + ch % CPR)
                  : vec_t{};
    }
  };
  if (r0 < r1) fetch(r0);
  for (int64_t e0 = r0; e0 < r1; e0 += SIG) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) {
      const int ch = tid + C::NTHR * t;
      if (ch < SIG * CPR) reinterpret_cast<vec_t*>(stage)[ch] = nx[t];
    }
    __syncthreads();
    if (e0 + SIG < r1) fetch(e0 + SIG);
    if constexpr (C::REUSE) {
      auto step = [&](auto wtag) {
#pragma unroll 2
        for (int k4 = 0; k4 < SIG; k4 += 4)
          big_gram_step<T, NT, decltype(wtag)::value>(acc, stage + (k4 + kk) * KP + cl, T(1));
      };
      dispatch_wave<NW>(wv, step);
    } else {
      for (int k4 = 0; k4 < SIG; k4 += 4) {
        const T* yk = stage + (k4 + kk) * KP + cl;
#pragma unroll
        for (int s = 0; s < TPW; ++s)
          if (TI[s] >= 0) acc[s] = M::mma(yk[16 * TI[s]], yk[16 * TJ[s]], acc[s]);
      }
    }
  }
  double* out = partial + (int64_t)blockIdx.x * NTT * 256;
#pragma unroll
  for (int s = 0; s < TPW; ++s) {
    if (TI[s] >= 0) {
      const int t = tile_index(TI[s], TJ[s]);
#pragma unroll
      for (int r = 0; r < 4; ++r) out[t * 256 + M::crow(lane, r) * 16 + cl] = (double)acc[s][r];
    }
  }
}

// gram_reduce_kernel (wals.hip) with the tile count at run time: the same chunks in the same
// order, one kernel for every tiling
template <typename T>
__global__ __launch_bounds__(256) void gram_reduce_rt_kernel(const double* partial, int nblocks,
                                                             int nt, T* G) {
  __shared__ double red[16][16];
  const int KP = 16 * nt;
  const int NTT = nt * (nt + 1) / 2;
  const int o = threadIdx.x & 15, ch = threadIdx.x >> 4;
  const int idx = blockIdx.x * 16 + o;
  const int i = idx / KP, j = idx % KP;
  const int ii = i >= j ? i : j, jj = i >= j ? j : i;
  const int t = tile_index(ii >> 4, jj >> 4);
  const int off = t * 256 + (ii & 15) * 16 + (jj & 15);
  const double s = gram_reduce_one(partial, nblocks, (int64_t)NTT * 256, off, red, o, ch);
  if (ch == 0) G[idx] = (T)s;
}

#ifndef QMFX_KERNELS_ONLY
template <typename T>
static hipError_t gram_big(const T* Y, int64_t n, int nt, T* G, double* partial, int max_blocks,
                           hipStream_t s) {
  int64_t rpb = (n + max_blocks - 1) / max_blocks;
  rpb = ((rpb + 3) / 4) * 4;
  if (rpb < 64) rpb = 64;
  const int nblocks = (int)((n + rpb - 1) / rpb);
  const hipError_t e = dispatch_nt<big_gram_min_nt(sizeof(T)), kBigMaxNT>(nt, [&](auto N) {
    constexpr int NT = decltype(N)::value;
    if (nblocks > 0)
      hipLaunchKernelGGL((gram_tiles_kernel<T, NT>), dim3(nblocks), dim3(BigCfg<T, NT>::NTHR), 0,
                         s, Y, n, rpb, partial);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  const int KP = 16 * nt;
  hipLaunchKernelGGL((gram_reduce_rt_kernel<T>), dim3(KP * KP / 16), dim3(256), 0, s,
                     partial, nblocks, nt, G);
  return hipGetLastError();
}
hipError_t launch_gram_big(const float* Y, int64_t n, int nt, float* G, double* partial,
                           int max_blocks, hipStream_t s) {
  return gram_big(Y, n, nt, G, partial, max_blocks, s);
}
hipError_t launch_gram_big(const double* Y, int64_t n, int nt, double* G, double* partial,
                           int max_blocks, hipStream_t s) {
  return gram_big(Y, n, nt, G, partial, max_blocks, s);
}
#endif  // QMFX_KERNELS_ONLY

}  // namespace qmfx
