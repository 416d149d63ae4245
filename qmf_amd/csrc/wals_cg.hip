// Conjugate-gradient row solves of a WALS half (qmfx_wals_half_cg; contract in include/qmfx.h).
//
// Row r with signals (j_e, v_e) solves A·x = b, A = G + Σ_e w_e·y_e·y_eᵀ + λI, b = Σ_e c_e·y_e
// (w = αv, c = 1 + αv, y_e = row j_e of the fixed side, G = YᵀY), by `steps` CG steps from the
// row's current value.  A is never formed: one operator application is G·v, a gather pass
// over the row's signals, and λ·v.
//
// A workgroup of 4 waves owns kCgRows = 16 rows (slots of the side's order, so the rows of a
// block have similar lengths).  The block's vectors P, Q, R and b live in LDS as 16 × KP
// matrices; x stays in the factor matrix itself (the owning lanes update it in place).  Per
// operator application:
//   1. Q = P·G for the whole block on the matrix cores (16x16x4 MFMA of the context precision):
//      wave w owns the column tiles w, w + 4, …; G is streamed from L2 once per block, not once
//      per row.
//   2. each wave adds the sparse term and λ·p for its 4 rows (w, w + 4, …), one row at a time:
//      16 lanes per signal, 4 signals per pass; lane s of a group holds the factors s + 16m.
//      The gathered rows come from L2 / Infinity Cache on every application (nothing is staged
//      across steps), so a row of any length takes the same path.
// Dot products of a signal are in T; ρ, d, Σc and the loss are accumulated in double in both
// precisions.  All reductions run in a fixed order: two calls from one state give the same bits.
//
// Rows of the split-K heavy class never come here: the host sends them to the exact heavy-row
// launcher (one wave must not serialise a million gathers per step; they are few, and the exact
// solve is CG's limit).
#include "common.h"
#include "kernels.h"
#include "ntswitch.h"

namespace qmfx {

namespace {

constexpr int CG_WAVES = 4, CG_THREADS = 64 * CG_WAVES, CG_RPW = kCgRows / CG_WAVES;
static_assert(kCgRows == 16, "a block's rows are one MFMA tile");

// row stride of the LDS matrices: KP plus 4 dwords, so the MFMA operand read (16 rows × 4
// columns) and the 16-lane row reads touch every bank once
template <typename T>
constexpr int cg_ld(int kp) {
  return kp + 16 / (int)sizeof(T);
}

// sum over the 16 lanes of a signal group
template <typename V>
__device__ __forceinline__ V group_sum(V v) {
#pragma unroll
  for (int m = 1; m <= 8; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// sum over the 4 groups of a wave (lane s of each)
template <typename V>
__device__ __forceinline__ V cross_sum(V v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

template <typename T, int NT>
__global__ __launch_bounds__(CG_THREADS) void wals_cg_kernel(const CgArgs<T> a) {
  constexpr int KP = 16 * NT, LD = cg_ld<T>(KP), TPW = (NT + CG_WAVES - 1) / CG_WAVES;
  using acc_t = typename Mfma<T>::acc_t;
  extern __shared__ __align__(16) unsigned char cg_smem[];
  T* Pv = reinterpret_cast<T*>(cg_smem);
  T* Qv = Pv + kCgRows * LD;
  T* Rv = Qv + kCgRows * LD;
  T* Bv = Rv + kCgRows * LD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = lane & 15, g = lane >> 4;
  const int64_t slot0 = a.slot_begin + (int64_t)blockIdx.x * kCgRows;
  const int64_t slot_end = a.slot_begin + a.nslots;

  // wave-uniform state of this wave's rows
  int64_t beg[CG_RPW], xoff[CG_RPW];
  int n[CG_RPW], flag[CG_RPW];
  bool live[CG_RPW], active[CG_RPW];
  double rho[CG_RPW], csum[CG_RPW];
#pragma unroll
  for (int j = 0; j < CG_RPW; ++j) {
    const int i = wave + CG_WAVES * j;
    const int64_t slot = slot0 + i;
    const bool valid = slot < slot_end;
    RowDesc d{0, 0, 0};
    if (valid) d = a.desc[slot];
    beg[j] = d.beg;
    n[j] = d.n;
    xoff[j] = (int64_t)d.row * KP;
    live[j] = valid && d.n > 0;
    active[j] = live[j];
    flag[j] = 0;
    rho[j] = 0.0;
    csum[j] = 0.0;
    // x₀ → P; an empty row is exactly 0 with loss 0
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      const int f = s + 16 * m;
      const T x = live[j] ? a.X[xoff[j] + f] : T(0);
      if (g == 0) {
        Pv[i * LD + f] = x;
        if (valid && d.n == 0) a.X[xoff[j] + f] = T(0);
      }
    }
    if (valid && d.n == 0 && lane == 0) a.rowloss[d.row] = 0.0;
  }
  __syncthreads();

  // Q = P·G: C[i][j] = Σ_c P[i][c]·G[c][j], A operand from LDS, B operand from global
  auto gemm = [&]() {
    acc_t acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = acc_t{0, 0, 0, 0};
#pragma unroll 4
    for (int c = 0; c < KP / 4; ++c) {
      const T av = Pv[s * LD + 4 * c + g];
      const T* grow = a.G + (int64_t)(4 * c + g) * KP + s;
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const int jt = wave + CG_WAVES * t;
        if (jt < NT) acc[t] = Mfma<T>::mma(av, grow[16 * jt], acc[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int jt = wave + CG_WAVES * t;
      if (jt < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Qv[Mfma<T>::crow(lane, r) * LD + 16 * jt + s] = acc[t][r];
      }
    }
  };

  // q = Q[i] + Σ_e w_e·(y_e·p)·y_e + λ·p for row j of this wave, p = P[i]; with FIRST also
  // b = Σ_e c_e·y_e and Σc.  Every lane ends with q (and b) of its factors s + 16m.
  auto apply_row = [&](int j, auto first, T (&p)[NT], T (&q)[NT], T (&b)[NT]) {
    constexpr bool FIRST = decltype(first)::value;
    const int i = wave + CG_WAVES * j;
    T acc[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      p[m] = Pv[i * LD + s + 16 * m];
      acc[m] = T(0);
      if constexpr (FIRST) b[m] = T(0);
    }
    double cs = 0.0;
    const int nn = n[j];
    const int32_t* col = a.col + beg[j];
    const T* val = a.val + beg[j];
    int cj = g < nn ? col[g] : 0;
    T v = g < nn ? val[g] : T(0);
    for (int e0 = 0; e0 < nn; e0 += 4) {
      const bool ok = e0 + g < nn;
      const T* yr = a.Y + (int64_t)cj * KP + s;
      T y[NT];
#pragma unroll
      for (int m = 0; m < NT; ++m) y[m] = ok ? yr[16 * m] : T(0);
      const T w = a.alpha * v;
      // the next pass's signal
      const int en = e0 + 4 + g;
      cj = en < nn ? col[en] : 0;
      v = en < nn ? val[en] : T(0);
      T dot = T(0);
#pragma unroll
      for (int m = 0; m < NT; ++m) dot += y[m] * p[m];
      dot = group_sum(dot);
      const T coef = w * dot;
#pragma unroll
      for (int m = 0; m < NT; ++m) acc[m] += coef * y[m];
      if constexpr (FIRST) {
        const T cc = T(1) + w;
#pragma unroll
        for (int m = 0; m < NT; ++m) b[m] += cc * y[m];
        if (ok) cs += (double)cc;
      }
    }
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      q[m] = Qv[i * LD + s + 16 * m] + cross_sum(acc[m]) + a.lambda * p[m];
      if constexpr (FIRST) b[m] = cross_sum(b[m]);
    }
    if constexpr (FIRST) csum[j] = cross_sum(cs);
  };

  // r = b − A·x₀, p = r, ρ = r·r
  gemm();
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CG_RPW; ++j) {
    if (!live[j]) continue;
    const int i = wave + CG_WAVES * j;
    T p[NT], q[NT], b[NT];
    apply_row(j, std::true_type{}, p, q, b);
    double rr = 0.0;
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      const T r = b[m] - q[m];
      rr += (double)r * (double)r;
      if (g == 0) {
        const int f = s + 16 * m;
        Rv[i * LD + f] = r;
        Pv[i * LD + f] = r;
        Bv[i * LD + f] = b[m];
      }
    }
    rho[j] = group_sum(rr);
  }
  __syncthreads();

  for (int t = 0; t < a.steps; ++t) {
    gemm();
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CG_RPW; ++j) {
      if (!active[j]) continue;
      if (rho[j] == 0.0) {
        active[j] = false;
        continue;
      }
      const int i = wave + CG_WAVES * j;
      T p[NT], q[NT], b[NT];
      apply_row(j, std::false_type{}, p, q, b);
      double dd = 0.0;
#pragma unroll
      for (int m = 0; m < NT; ++m) dd += (double)p[m] * (double)q[m];
      const double d = group_sum(dd);
      if (!(d > 0.0)) {
        // not positive definite along p (or NaN): the row keeps its last iterate
        flag[j] = 1;
        active[j] = false;
        continue;
      }
      const T al = (T)(rho[j] / d);
      T r[NT];
      double rr = 0.0;
#pragma unroll
      for (int m = 0; m < NT; ++m) {
        r[m] = Rv[i * LD + s + 16 * m] - al * q[m];
        rr += (double)r[m] * (double)r[m];
      }
      const double rho1 = group_sum(rr);
      const T beta = (T)(rho1 / rho[j]);
      rho[j] = rho1;
      if (g == 0) {
#pragma unroll
        for (int m = 0; m < NT; ++m) {
          const int f = s + 16 * m;
          a.X[xoff[j] + f] += al * p[m];
          Rv[i * LD + f] = r[m];
          Pv[i * LD + f] = r[m] + beta * p[m];
        }
      }
    }
    __syncthreads();
  }

  // loss on the stored iterate with A·x = b − r: Σc − x·b − x·r − λ·x·x
#pragma unroll
  for (int j = 0; j < CG_RPW; ++j) {
    if (!live[j]) continue;
    const int i = wave + CG_WAVES * j;
    double xb = 0.0, xr = 0.0, xx = 0.0;
    if (g == 0) {
      // the lanes that updated x read it back
#pragma unroll
      for (int m = 0; m < NT; ++m) {
        const int f = s + 16 * m;
        const double x = (double)a.X[xoff[j] + f];
        xb += x * (double)Bv[i * LD + f];
        xr += x * (double)Rv[i * LD + f];
        xx += x * x;
      }
    }
    xb = group_sum(xb);
    xr = group_sum(xr);
    xx = group_sum(xx);
    if (lane == 0) {
      const int64_t row = xoff[j] / KP;
      a.rowloss[row] = csum[j] - xb - xr - (double)a.lambda * xx;
      if (flag[j]) a.status[row] = 1;
    }
  }
}

template <typename T>
hipError_t cg(const CgArgs<T>& a, int nt, hipStream_t st) {
  if (a.nslots <= 0) return hipSuccess;
  return dispatch_nt<1, kCgMaxNT>(nt, [&](auto ntc) {
    constexpr int NT = decltype(ntc)::value;
    const size_t lds = (size_t)4 * kCgRows * cg_ld<T>(16 * NT) * sizeof(T);
    const void* fn = (const void*)wals_cg_kernel<T, NT>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    // a launch's thread count must fit 32 bits
    const int64_t cap = (((int64_t)1 << 31) / CG_THREADS - 1) * kCgRows;
    for (int64_t done = 0; done < a.nslots; done += cap) {
      CgArgs<T> c = a;
      c.slot_begin = a.slot_begin + done;
      c.nslots = a.nslots - done < cap ? a.nslots - done : cap;
      const dim3 grid((unsigned)((c.nslots + kCgRows - 1) / kCgRows)), block(CG_THREADS);
      hipLaunchKernelGGL((wals_cg_kernel<T, NT>), grid, block, lds, st, c);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  });
}

}  // namespace

hipError_t launch_wals_cg(const CgArgs<float>& a, int nt, hipStream_t s) { return cg(a, nt, s); }
hipError_t launch_wals_cg(const CgArgs<double>& a, int nt, hipStream_t s) { return cg(a, nt, s); }

}  // namespace qmfx
