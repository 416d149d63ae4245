// The screen of qmfx_recommend_screened: an f32 MFMA scan of the whole catalogue whose epilogue
// keeps, per requested user, the items that a certified bound cannot rule out of the user's
// exact top-N.  Only those are scored exactly afterwards (cand_select_kernel, recommend.hip).
//
//   screen_gather_kernel  the requested users' rows, dense [nreq][kp] in the context precision
//                         (requests repeat and come in any order);
//   screen_f32_kernel     an fp64 context's rows rounded to f32 (users: the gathered rows; items:
//                         the whole matrix).  An fp32 context is scanned as it is;
//   screen_prep_kernel    the threshold L_u of every user from the exact top-N of the sample
//                         (+inf when the sample gave fewer than N eligible items: nothing finite
//                         passes, the host sends the user to the exact scan), the pass counters
//                         zeroed and the sample's counts kept;
//   screen_kernel         grid (item tiles, user tiles) of 128 × 128, 4 waves of 64 × 64: the
//                         operands staged through LDS in 32-column stages, transposed to [column]
//                         [row] so that an MFMA operand read is 32 consecutive floats;
//                         v_mfma_f32_32x32x2_f32 accumulates a(u, i), an f32 fma chain in factor
//                         order from 0.  Epilogue: item i passes for user u unless a is finite and
//                         a + b_i < L_u − ε(u, i) in double (include/qmfx.h states ε and DESIGN
//                         §3.12 proves it); a passing item takes the next slot of the user's list
//                         through an atomicAdd on the user's counter.  The counter keeps running
//                         past the list's capacity (the overflow signal), stores stop there.
//                         Rows beyond the request or the catalogue are staged as zeros and masked
//                         in the epilogue; columns at or beyond k are staged as zeros;
//   screen_keys_kernel    the kept lists as keys (position in the request) << 32 | item at their
//                         place in the packed candidate array; data.hip's radix sort orders them
//                         and screen_unpack_kernel takes the items back out: every list ascending,
//                         as qmfx_recommend_candidates' lists are.
//
// LDS of screen_kernel: 2 × 32 × 132 × 4 B = 33,792 B (the epilogue's per-user values reuse it).
#include "common.h"
#include "kernels.h"

namespace qmfx {
namespace {

constexpr int SC_TU = kScreenTileUsers;  // users per workgroup
constexpr int SC_TI = kScreenTileItems;  // items per workgroup
constexpr int SC_KC = 32;                // factor columns per LDS stage
constexpr int SC_LD = 128 + 4;           // LDS row stride in floats (a row: one column's 128 values)
static_assert(SC_TU == 128 && SC_TI == 128, "4 waves of 64 × 64, staged 32 rows per pass");

// ε(u, i) = SC_REL(k) · ‖u‖‖q_i‖ + SC_BIAS(k) · |b_i| + SC_ABS · (1 + ‖u‖ + ‖q_i‖)   (include/qmfx.h)
__device__ __forceinline__ double sc_rel(int k) { return (double)(k + 4) * 0x1p-23; }
__device__ __forceinline__ double sc_bias(int k) { return (double)(k + 4) * 0x1p-52; }
constexpr double SC_ABS = 0x1p-116;

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename T>
__global__ __launch_bounds__(256) void screen_gather_kernel(const T* __restrict__ U,
                                                            const int64_t* __restrict__ users,
                                                            int64_t nreq, int kp,
                                                            T* __restrict__ out) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= nreq * kp) return;
  const int64_t t = x / kp;
  out[x] = U[users[t] * kp + (x - t * kp)];
}

__global__ __launch_bounds__(256) void screen_f32_kernel(const double* __restrict__ in, int64_t n,
                                                         float* __restrict__ out) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x < n) out[x] = (float)in[x];  // round to nearest even
}

__global__ __launch_bounds__(256) void screen_prep_kernel(const double* __restrict__ scores,
                                                          const int32_t* __restrict__ counts,
                                                          int64_t nreq, int topn,
                                                          double* __restrict__ thr,
                                                          int32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ scnt) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nreq) return;
  const int32_t n = counts[t];
  thr[t] = n == topn ? scores[t * topn + topn - 1] : __builtin_inf();
  cnt[t] = 0;
  scnt[t] = n;
}

template <typename T>
__global__ __launch_bounds__(256) void screen_kernel(ScreenArgs<T> a) {
  __shared__ __attribute__((aligned(16))) float sA[SC_KC * SC_LD];
  __shared__ __attribute__((aligned(16))) float sB[SC_KC * SC_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wu = w >> 1, wi = w & 1;  // this wave's 64 users × 64 items of the tile
  // tiles in one grid dimension, item tiles fastest (neighbours share the users' rows)
  const int64_t by = blockIdx.x / a.itiles, bx = blockIdx.x - by * a.itiles;
  const int64_t u0 = by * SC_TU, i0 = bx * SC_TI;

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  const int kq = tid & 7;   // the thread's four columns of a stage
  const int sr = tid >> 3;  // its row of every 32-row pass
  for (int f0 = 0; f0 < a.kp; f0 += SC_KC) {
    const int kend = a.kp - f0 < SC_KC ? a.kp - f0 : SC_KC;  // a multiple of 16
    const int c = f0 + 4 * kq;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < SC_TU / 32; ++p) {
      const int r = sr + 32 * p;
      float4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (c < a.kp) {  // kp is a multiple of 16: the four columns are inside the row or beyond it
        if (u0 + r < a.nreq) va = *(const float4*)(a.A + (u0 + r) * a.kp + c);
        if (i0 + r < a.nitems) vb = *(const float4*)(a.B + (i0 + r) * a.kp + c);
      }
      const float xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = c + j < a.k;
        sA[(4 * kq + j) * SC_LD + r] = live ? xa[j] : 0.f;
        sB[(4 * kq + j) * SC_LD + r] = live ? xb[j] : 0.f;
      }
    }
    __syncthreads();
    // 32x32x2: lane l supplies A[row l & 31][column l >> 5] and B[column l >> 5][row l & 31]
    for (int kk = 0; kk < kend; kk += 2) {
      const int kr = (kk + (lane >> 5)) * SC_LD + (lane & 31);
      float af[2], bf[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) af[m] = sA[kr + wu * 64 + m * 32];
#pragma unroll
      for (int n = 0; n < 2; ++n) bf[n] = sB[kr + wi * 64 + n * 32];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m], bf[n], acc[m][n], 0, 0, 0);
    }
  }

  // the tile's users through LDS (the staging buffers are free): threshold, c_rel·‖u‖, c_abs·‖u‖
  __syncthreads();
  double* const sL = (double*)sA;  // [128]
  double* const sRu = sL + SC_TU;  // [128]
  double* const sCu = (double*)sB;  // [128]
  if (tid < SC_TU) {
    const int64_t u = u0 + tid;
    const double nu = u < a.nreq ? a.unorm[u] : 0.0;
    sL[tid] = u < a.nreq ? a.thr[u] : __builtin_inf();
    sRu[tid] = sc_rel(a.k) * nu;
    sCu[tid] = SC_ABS * nu;
  }
  __syncthreads();

  // accumulator register r of lane l: user row 8·(r / 4) + 4·(l >> 5) + r % 4, item column l & 31
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int64_t item = i0 + wi * 64 + n * 32 + (lane & 31);
    const bool ivalid = item < a.nitems;
    const double nq = ivalid ? a.inorm[item] : 0.0;
    const double b = (ivalid && a.bias) ? (double)a.bias[item] : 0.0;
    // the item's share of ε: c_bias·|b| + c_abs·(1 + ‖q‖)
    const double ti = sc_bias(a.k) * __builtin_fabs(b) + SC_ABS * (1.0 + nq);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ul = wu * 64 + m * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        const int64_t u = u0 + ul;
        const float av = acc[m][n][r];
        // every term of ε is ≥ 0; L − ε and a + b are one rounding each, and rounding is monotone
        const double eps = __builtin_fma(sRu[ul], nq, ti + sCu[ul]);
        const bool drop = __builtin_isfinite(av) && ((double)av + b < sL[ul] - eps);
        if (ivalid && u < a.nreq && !drop) {
          const int32_t slot = atomicAdd(&a.cnt[u], 1);
          if (slot < a.cap) a.list[u * a.cap + slot] = (int32_t)item;
        }
      }
    }
  }
}

__global__ __launch_bounds__(64) void screen_keys_kernel(const int32_t* __restrict__ list,
                                                         const int64_t* __restrict__ cptr,
                                                         int64_t cap, uint64_t* __restrict__ keys) {
  const int64_t t = blockIdx.x;
  const int64_t b = cptr[t], n = cptr[t + 1] - b;  // 0: the user goes to the exact scan
  for (int64_t j = threadIdx.x; j < n; j += 64)
    keys[b + j] = ((uint64_t)t << 32) | (uint32_t)list[t * cap + j];
}

__global__ __launch_bounds__(256) void screen_unpack_kernel(const uint64_t* __restrict__ keys,
                                                            int64_t n, int32_t* __restrict__ cand) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x < n) cand[x] = (int32_t)(uint32_t)keys[x];
}

unsigned nb(int64_t n) { return (unsigned)((n + 255) / 256); }

template <typename T>
hipError_t screen(const ScreenArgs<T>& a0, hipStream_t s) {
  if (a0.nreq == 0 || a0.nitems == 0) return hipSuccess;
  ScreenArgs<T> a = a0;
  a.itiles = (a.nitems + SC_TI - 1) / SC_TI;
  const int64_t tiles = screen_tiles(a.nreq, a.nitems);
  if (tiles > kScreenMaxTiles || a.kp % 16 != 0 || a.cap < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(screen_kernel<T>, dim3((unsigned)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <typename T>
hipError_t gather(const T* U, const int64_t* users, int64_t nreq, int kp, T* out, hipStream_t s) {
  if (nreq == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_gather_kernel<T>, dim3(nb(nreq * kp)), dim3(256), 0, s, U, users, nreq,
                     kp, out);
  return hipGetLastError();
}

}  // namespace

int64_t screen_tiles(int64_t nreq, int64_t nitems) {
  return ((nreq + SC_TU - 1) / SC_TU) * ((nitems + SC_TI - 1) / SC_TI);
}
hipError_t launch_screen(const ScreenArgs<float>& a, hipStream_t s) { return screen(a, s); }
hipError_t launch_screen(const ScreenArgs<double>& a, hipStream_t s) { return screen(a, s); }
hipError_t launch_screen_gather(const float* U, const int64_t* users, int64_t nreq, int kp,
                                float* out, hipStream_t s) {
  return gather(U, users, nreq, kp, out, s);
}
hipError_t launch_screen_gather(const double* U, const int64_t* users, int64_t nreq, int kp,
                                double* out, hipStream_t s) {
  return gather(U, users, nreq, kp, out, s);
}
hipError_t launch_screen_f32(const double* in, int64_t n, float* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_f32_kernel, dim3(nb(n)), dim3(256), 0, s, in, n, out);
  return hipGetLastError();
}
hipError_t launch_screen_prep(const double* scores, const int32_t* counts, int64_t nreq, int topn,
                              double* thr, int32_t* cnt, int32_t* scnt, hipStream_t s) {
  if (nreq == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_prep_kernel, dim3(nb(nreq)), dim3(256), 0, s, scores, counts, nreq,
                     topn, thr, cnt, scnt);
  return hipGetLastError();
}
hipError_t launch_screen_keys(const int32_t* list, const int64_t* cptr, int64_t nreq, int64_t cap,
                              uint64_t* keys, hipStream_t s) {
  if (nreq == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_keys_kernel, dim3((unsigned)nreq), dim3(64), 0, s, list, cptr, cap,
                     keys);
  return hipGetLastError();
}
hipError_t launch_screen_unpack(const uint64_t* keys, int64_t n, int32_t* cand, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_unpack_kernel, dim3(nb(n)), dim3(256), 0, s, keys, n, cand);
  return hipGetLastError();
}

}  // namespace qmfx
