// WALS whitened (n×n Woodbury) row kernels on MI355X (gfx950).  See wals.hip for the per-row
// algebra, whiten.hip for the whitening GEMMs around them and chol_inv.hip for their L⁻¹.
//
// Reference path (taozhijiang/qmf): WALSEngine::updateFactorsForOne
// qmf/wals/WALSEngine.cpp:266-310 and linearSymmetricSolve qmf/Matrix.cpp:81-96 (the same
// solution by the push-through identity).
#include <type_traits>

#include "chol.h"
#include "common.h"
#include "kernels.h"
#include "ntswitch.h"
#include "rowsolve.h"

namespace qmfx {

// ---------------------------------------------------------------------------------------
// Whitened row kernel (n ≤ 16·NTN signals, n ≤ KP/2).  One wave64 per row.  The row's
// whitened fixed-side rows z_e (KP values each) are loaded ONCE into registers in MFMA
// operand order (lane (i, g) holds z_{16I+i}[16q + 4g .. +3] for every I, q), so that
//   K = Zₛ Zₛᵀ         — NTN(NTN+1)/2 tiles × KP/4 steps of 16x16x4 MFMA from registers,
//   x' = Zₛᵀu, Zₛᵀc   — per-lane FMAs + 16-lane DPP row sums,
// and the HBM traffic per signal is one gathered row, as in the direct kernel.
// Writes x' (whitened); whiten_kernel<UNWHITEN> maps it to x = L⁻ᵀ x' and adds −λ‖x‖².
// ---------------------------------------------------------------------------------------
// fp64 k ≤ 48 only (NTN = 1): fp32 and fp64 k ≥ 64 run the streamed kernels below.
template <int NTK, int NTN, bool TRACE>
__global__ __launch_bounds__(64, 2) void wals_woodbury_kernel(SolveArgs<double> a) {
  using T = double;
  using M = Mfma<T>;
  using acc_t = typename M::acc_t;
  using v4 = typename M::acc_t;  // 4-wide vector of T
  constexpr int KP = 16 * NTK;
  constexpr int NTT = NTN * (NTN + 1) / 2;
  __shared__ __attribute__((aligned(16))) CholShared<T, NTN> S;
  __shared__ __attribute__((aligned(16))) T gq[16 * NTN];

  // one row per wave: the slot's descriptor, then its signals (lane = signal)
  const int lane = threadIdx.x;
  const int cl = lane & 15;
  const int kk = lane >> 4;
  const int64_t i = blockIdx.x;
  const RowDesc dn = a.desc[a.row_begin + i];
  const int64_t row = dn.row;
  const int n = dn.n;  // ≤ 16·NTN by bucketing
  uint64_t tr[5] = {0, 0, 0, 0, 0};
  if (TRACE) tr[0] = __builtin_amdgcn_s_memtime();

  // signal e = lane: column, weight, confidence
  const bool mine = lane < n;
  const int cr = mine ? a.col[dn.beg + lane] : a.zrow;
  const T vr = mine ? a.val[dn.beg + lane] : T(0);
  const T wl = mine ? a.alpha * vr : T(0);
  const T cwl = mine ? T(1) + a.alpha * vr : T(0);
  const bool isP = mine && wl > T(0);
  const bool isQ = mine && wl == T(0);
  int bad = __any(mine && wl < T(0)) ? 1 : 0;  // negative confidence: not SPD in this form
  const uint64_t mQ = __ballot(isQ);
  const bool hasQ = mQ != 0;

  // gather Zₛ into registers: zr[I][q] = z_{16I+cl}[16q + 4kk .. +3].  Padding signals
  // (e ≥ n) load the all-zero row a.zrow, so their K rows and columns are exactly 0.
  v4 zr[NTN][NTK];
#pragma unroll
  for (int I = 0; I < NTN; ++I) {
    const int ce = __shfl(cr, 16 * I + cl, 64);
    const v4* zrow = reinterpret_cast<const v4*>(a.Y + (uint64_t)(uint32_t)ce * KP) + kk;
#pragma unroll
    for (int q = 0; q < NTK; ++q) zr[I][q] = zrow[4 * q];
  }
  if (TRACE) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    tr[1] = __builtin_amdgcn_s_memtime();
  }
  // K = Zₛ Zₛᵀ (lower tiles); the summation index j = 16q + 4kk + comp is the same for the
  // A and B operands, so its order within a step does not matter
  acc_t acc[NTT];
#pragma unroll
  for (int t = 0; t < NTT; ++t) acc[t] = acc_t{0, 0, 0, 0};
  {
#pragma unroll
    for (int q = 0; q < NTK; ++q) {
#pragma unroll
      for (int comp = 0; comp < 4; ++comp) {
#pragma unroll
        for (int I = 0; I < NTN; ++I) {
#pragma unroll
          for (int J = 0; J <= I; ++J) {
            const int t = tile_index(I, J);
            acc[t] = M::mma(zr[I][q][comp], zr[J][q][comp], acc[t]);
          }
        }
      }
    }
  }
  double xb = 0.0;  // xᵀb of the row (= x'ᵀ Zₛᵀc)
  T ul[NTN];        // u of signal 16I + cl
  if (!hasQ) {
    // Every real signal is in P.  S = W⁻¹ + K on all 16·NTN slots: padding slots have
    // K = 0 (zero rows) and take W⁻¹ = 1, so S is the identity there and u = 0.
    const T iw = isP ? fast_rcp(wl) : T(1);
    const T rhs = isP ? cwl * iw : T(0);
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const T iwd = __shfl(iw, 16 * I + cl, 64);  // diagonal (e, e), e = 16I + cl
      const int t = tile_index(I, I);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] += M::crow(lane, r) == cl ? iwd : T(0);
    }
    if (lane < 16 * NTN) S.bw[lane] = rhs;
    __syncthreads();
    if (TRACE) tr[2] = __builtin_amdgcn_s_memtime();
    chol_solve<T, NTN>(acc, S, lane, bad);
    if (TRACE) tr[3] = __builtin_amdgcn_s_memtime();
    // xᵀb = uᵀK c = cᵀ(r − W⁻¹u) = Σ_e (c_e/w_e)(c_e − u_e)   (S u = r, r = W⁻¹c)
    const T ue = lane < 16 * NTN ? S.xs[lane] : T(0);
    xb = wave_sum(isP ? (double)(rhs * (cwl - ue)) : 0.0);
#pragma unroll
    for (int I = 0; I < NTN; ++I) ul[I] = S.xs[16 * I + cl];
  } else {
    // General row (some signals with v = 0: c = 1, w = 0, the set Q):
    // (W_P⁻¹ + K_PP) u_P = W_P⁻¹ c_P − K_PQ 1_Q,  u_Q = 1,  kq_e = z_eᵀ Σ_{f∈Q} z_f
    T rhs = isP ? cwl * fast_rcp(wl) : T(0);
    {
      T gpart[NTK][4];
#pragma unroll
      for (int q = 0; q < NTK; ++q)
#pragma unroll
        for (int comp = 0; comp < 4; ++comp) gpart[q][comp] = T(0);
#pragma unroll
      for (int I = 0; I < NTN; ++I) {
        const bool qe = (mQ >> (16 * I + cl)) & 1;
#pragma unroll
        for (int q = 0; q < NTK; ++q)
#pragma unroll
          for (int comp = 0; comp < 4; ++comp)
            if (qe) gpart[q][comp] += zr[I][q][comp];
      }
#pragma unroll
      for (int q = 0; q < NTK; ++q) row16_sum4(gpart[q]);
#pragma unroll
      for (int I = 0; I < NTN; ++I) {
        T sq = T(0);
#pragma unroll
        for (int q = 0; q < NTK; ++q)
#pragma unroll
          for (int comp = 0; comp < 4; ++comp) sq += zr[I][q][comp] * gpart[q][comp];
        sq += shfl_xor(sq, 16);
        sq += shfl_xor(sq, 32);
        if (kk == 0) gq[16 * I + cl] = sq;
      }
      __syncthreads();
      const T kqv = lane < 16 * NTN ? gq[lane] : T(0);
      if (isP) rhs -= kqv;
    }
    // S = W_P⁻¹ + K_PP on P×P, identity elsewhere (Q rows and padding)
    const T iw = isP ? fast_rcp(wl) : T(0);
    const uint64_t mP = __ballot(isP);
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      // the diagonal element (e, e), e = 16I + cl, sits in this lane's column cl
      const T iwd = __shfl(iw, 16 * I + cl, 64);
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        const int t = tile_index(I, J);
        const int f = 16 * J + cl;
        const bool pf = (mP >> f) & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = 16 * I + M::crow(lane, r);
          const bool pe = (mP >> e) & 1;
          T v = acc[t][r];
          if (pe && pf) v += (e == f) ? iwd : T(0);
          else v = (e == f) ? T(1) : T(0);
          acc[t][r] = v;
        }
      }
    }
    if (lane < 16 * NTN) S.bw[lane] = rhs;
    __syncthreads();
    if (TRACE) tr[2] = __builtin_amdgcn_s_memtime();
    chol_solve<T, NTN>(acc, S, lane, bad);
    if (TRACE) tr[3] = __builtin_amdgcn_s_memtime();
    // u_e: solved for P, 1 for Q (c = 1), 0 for padding
    T cv[NTN];
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const int e = 16 * I + cl;
      const bool pe = (mP >> e) & 1;
      const bool qe = (mQ >> e) & 1;
      ul[I] = pe ? S.xs[e] : (qe ? T(1) : T(0));
      cv[I] = __shfl(cwl, e, 64);
    }
    // xᵀb = x'ᵀ(Zₛᵀc)
#pragma unroll
    for (int q = 0; q < NTK; ++q) {
      T sx[4], sb[4];
#pragma unroll
      for (int comp = 0; comp < 4; ++comp) {
        sx[comp] = T(0);
        sb[comp] = T(0);
#pragma unroll
        for (int I = 0; I < NTN; ++I) {
          sx[comp] += zr[I][q][comp] * ul[I];
          sb[comp] += zr[I][q][comp] * cv[I];
        }
      }
      row16_sum4(sx);
      row16_sum4(sb);
#pragma unroll
      for (int comp = 0; comp < 4; ++comp) xb += (double)sx[comp] * (double)sb[comp];
    }
    xb = wave_sum(cl == 0 ? xb : 0.0);
  }
  // x' = Zₛᵀ u, column j = 16q + 4kk + comp; lane cl == q of each group stores its 4
  // columns (a failed row stores x' = 0, so x = 0 and its loss term is 0; the host
  // re-solves it)
#pragma unroll
  for (int q = 0; q < NTK; ++q) {
    T xq[4];
#pragma unroll
    for (int comp = 0; comp < 4; ++comp) {
      T sx = T(0);
#pragma unroll
      for (int I = 0; I < NTN; ++I) sx += zr[I][q][comp] * ul[I];
      xq[comp] = sx;
    }
    row16_sum4(xq);
    if (cl == q) {
      v4 o = {xq[0], xq[1], xq[2], xq[3]};
      if (bad) o = v4{};
      reinterpret_cast<v4*>(a.X + row * KP)[4 * q + kk] = o;
    }
  }
  const double csum = wave_sum((double)cwl);
  if (lane == 0) {
    a.rowloss[row] = bad ? 0.0 : csum - xb;  // −λ‖x‖² added after unwhitening
    if (bad && a.status) a.status[row] = 1;
  }
  if (TRACE && lane == 0) {
    tr[4] = __builtin_amdgcn_s_memtime();
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    uint64_t* o = a.trace + 8 * (a.row_begin + i);
#pragma unroll
    for (int j = 0; j < 5; ++j) o[j] = tr[j];
    o[5] = hw | ((uint64_t)xcc << 32);
    o[6] = (uint64_t)n;
    o[7] = (uint64_t)row;
  }
}

// ---------------------------------------------------------------------------------------
// Whitened row kernel, streamed (fp32, k ≤ 128): the n×n solve of wals_woodbury_kernel
// without holding Zₛ in registers.  K = Zₛ Zₛᵀ accumulates over 32-column chunks of the
// gathered rows — each chunk split into bf16 parts as it arrives, the next chunk in flight —
// and x' = Zₛᵀu gathers the rows a second time after the solve, from the L2 / MALL (the same
// rows were read a few µs earlier).  Lane (i, g) holds columns 32s + 8g .. +7 of signal
// 16I + i in chunk s.  ≈150 VGPRs instead of 256 at NTN = 4: three waves per SIMD.
// ---------------------------------------------------------------------------------------
// K on the bf16 matrix cores from split3 parts (the exact f32 MFMA path measured slower at
// k = 64 and 128: profiles/r06/ab_c2_f32_kpass.txt)
// What the bucket n ≤ 16·NTN is compiled with.
template <int NTN>
struct WbStCfg {
  static_assert(NTN >= 1 && NTN <= 8);
  //                                  NTN = 1  2  3  4  5  6  7  8
  // waves per SIMD: the n×n buckets beyond 64 signals (NTN = 5..8, k = 128 / 256) carry H = 2
  // signals per lane (e = lane and lane + 64), and the registers of the wider tiles leave
  // two or one waves
  static constexpr int WAVES_T[8] = {3, 3, 3, 3, 2, 1, 1, 1};
  static constexpr int H_T[8]     = {1, 1, 1, 1, 2, 2, 2, 2};
  // chunks in flight ahead of the one being consumed, K pass and x' pass
  static constexpr int KD_T[8]    = {1, 1, 1, 1, 1, 1, 1, 1};
  static constexpr int XD_T[8]    = {1, 1, 1, 1, 1, 1, 1, 1};
  static constexpr int WAVES = WAVES_T[NTN - 1];
  static constexpr int H = H_T[NTN - 1];
  static constexpr int KD = KD_T[NTN - 1];
  static constexpr int XD = XD_T[NTN - 1];
};
template <int NTK, int NTN>
__global__ __launch_bounds__(64, WbStCfg<NTN>::WAVES) void wals_woodbury_st_kernel(SolveArgs<float> a) {
  using C = WbStCfg<NTN>;
  using M = Mfma<float>;
  using acc_t = f32x4;
  constexpr int KP = 16 * NTK;
  constexpr int NTT = NTN * (NTN + 1) / 2;
  constexpr int NS = (KP + 31) / 32;
  __shared__ __attribute__((aligned(16))) CholShared<float, NTN> S;
  __shared__ __attribute__((aligned(16))) float gq[16 * NTN];

  constexpr int H = C::H;  // signals per lane: e = lane + 64h
  const int lane = threadIdx.x;
  const int cl = lane & 15;
  const int kk = lane >> 4;
  const RowDesc dn = a.desc[a.row_begin + blockIdx.x];
  const int64_t row = dn.row;
  const int n = dn.n;  // ≤ 16·NTN by bucketing
  bool mine[H], isP[H], isQ[H];
  int cr[H];
  float wl[H], cwl[H];
  uint64_t mQ[H];
  int bad = 0;
  bool hasQ = false;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const int e = lane + 64 * h;
    mine[h] = e < n;
    cr[h] = mine[h] ? a.col[dn.beg + e] : a.zrow;
    const float vr = mine[h] ? a.val[dn.beg + e] : 0.f;
    wl[h] = mine[h] ? a.alpha * vr : 0.f;
    cwl[h] = mine[h] ? 1.f + a.alpha * vr : 0.f;
    isP[h] = mine[h] && wl[h] > 0.f;
    isQ[h] = mine[h] && wl[h] == 0.f;
    bad |= __any(mine[h] && wl[h] < 0.f) ? 1 : 0;
    mQ[h] = __ballot(isQ[h]);
    hasQ |= mQ[h] != 0;
  }
  // bit e of a per-signal mask held as H 64-bit words
  auto bit = [](const uint64_t (&m)[H], int e) -> bool { return (m[e >> 6] >> (e & 63)) & 1; };

  // this lane's signals 16I + cl (padding signals read the all-zero row a.zrow)
  const f32x4* zp[NTN];
#pragma unroll
  for (int I = 0; I < NTN; ++I) {
    const int ce = __shfl(cr[I >> 2], (16 * I + cl) & 63, 64);
    zp[I] = reinterpret_cast<const f32x4*>(a.Y + (uint64_t)(uint32_t)ce * KP);
  }
  auto load_chunk = [&](int s, f32x4 (&buf)[NTN][2]) {
    const int c4 = 8 * s + 2 * kk;  // f32x4 index of column 32s + 8kk
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      if (32 * s + 32 <= KP || 32 * s + 8 * kk < KP) {
        buf[I][0] = zp[I][c4];
        buf[I][1] = zp[I][c4 + 1];
      } else {
        buf[I][0] = f32x4{0.f, 0.f, 0.f, 0.f};
        buf[I][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };

  acc_t acc[NTT];
#pragma unroll
  for (int t = 0; t < NTT; ++t) acc[t] = acc_t{0.f, 0.f, 0.f, 0.f};
  float sq[NTN];  // z_eᵀ Σ_{f∈Q} z_f over this lane's columns (rows with Q signals)
#pragma unroll
  for (int I = 0; I < NTN; ++I) sq[I] = 0.f;
  {
    // a ring of KD + 1 chunk buffers: chunk s + KD is in flight while chunk s is consumed
    constexpr int KD = C::KD;
    f32x4 buf[KD + 1][NTN][2];
#pragma unroll
    for (int s = 0; s < KD && s < NS; ++s) load_chunk(s, buf[s]);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s + KD < NS) load_chunk(s + KD, buf[(s + KD) % (KD + 1)]);
      f32x4 (&cur)[NTN][2] = buf[s % (KD + 1)];
      Split3 sp[NTN];
#pragma unroll
      for (int I = 0; I < NTN; ++I) {
        float x[8];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          x[c] = cur[I][0][c];
          x[4 + c] = cur[I][1][c];
        }
        split3(x, sp[I]);
      }
      if (hasQ) {
        float g[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float v = 0.f;
#pragma unroll
            for (int I = 0; I < NTN; ++I)
              if (bit(mQ, 16 * I + cl)) v += cur[I][h][c];
            g[h][c] = v;
          }
        row16_sum4(g[0]);
        row16_sum4(g[1]);
#pragma unroll
        for (int I = 0; I < NTN; ++I)
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < 4; ++c) sq[I] += cur[I][h][c] * g[h][c];
      }
#pragma unroll
      for (int I = 0; I < NTN; ++I) {
#pragma unroll
        for (int J = 0; J <= I; ++J) {
          const int t = tile_index(I, J);
          acc[t] = mma_split6(sp[I], sp[J], acc[t]);
        }
      }
      // one chunk's splits and the next chunks' loads live at a time
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  double xb = 0.0;
  float ul[NTN], cv[NTN];
  if (!hasQ) {
    float iw[H], rhs[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      iw[h] = isP[h] ? fast_rcp(wl[h]) : 1.f;
      rhs[h] = isP[h] ? cwl[h] * iw[h] : 0.f;
    }
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const float iwd = __shfl(iw[I >> 2], (16 * I + cl) & 63, 64);
      const int t = tile_index(I, I);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] += M::crow(lane, r) == cl ? iwd : 0.f;
    }
#pragma unroll
    for (int h = 0; h < H; ++h)
      if (lane + 64 * h < 16 * NTN) S.bw[lane + 64 * h] = rhs[h];
    __syncthreads();
    chol_solve<float, NTN>(acc, S, lane, bad);
    double xbl = 0.0;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float ue = lane + 64 * h < 16 * NTN ? S.xs[lane + 64 * h] : 0.f;
      xbl += isP[h] ? (double)(rhs[h] * (cwl[h] - ue)) : 0.0;
    }
    xb = wave_sum(xbl);
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      ul[I] = S.xs[16 * I + cl];
      cv[I] = 0.f;
    }
  } else {
    float rhs[H], iw[H];
#pragma unroll
    for (int h = 0; h < H; ++h) rhs[h] = isP[h] ? cwl[h] * fast_rcp(wl[h]) : 0.f;
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      float v = sq[I];
      v += shfl_xor(v, 16);
      v += shfl_xor(v, 32);
      if (kk == 0) gq[16 * I + cl] = v;
    }
    __syncthreads();
    uint64_t mP[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float kqv = lane + 64 * h < 16 * NTN ? gq[lane + 64 * h] : 0.f;
      if (isP[h]) rhs[h] -= kqv;
      iw[h] = isP[h] ? fast_rcp(wl[h]) : 0.f;
      mP[h] = __ballot(isP[h]);
    }
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const float iwd = __shfl(iw[I >> 2], (16 * I + cl) & 63, 64);
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        const int t = tile_index(I, J);
        const int f = 16 * J + cl;
        const bool pf = bit(mP, f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = 16 * I + M::crow(lane, r);
          const bool pe = bit(mP, e);
          float v = acc[t][r];
          if (pe && pf) v += (e == f) ? iwd : 0.f;
          else v = (e == f) ? 1.f : 0.f;
          acc[t][r] = v;
        }
      }
    }
#pragma unroll
    for (int h = 0; h < H; ++h)
      if (lane + 64 * h < 16 * NTN) S.bw[lane + 64 * h] = rhs[h];
    __syncthreads();
    chol_solve<float, NTN>(acc, S, lane, bad);
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const int e = 16 * I + cl;
      const bool pe = bit(mP, e);
      const bool qe = bit(mQ, e);
      ul[I] = pe ? S.xs[e] : (qe ? 1.f : 0.f);
      cv[I] = __shfl(cwl[I >> 2], e & 63, 64);
    }
  }

  // x' = Zₛᵀu (and for rows with Q signals xᵀb = x'ᵀ(Zₛᵀc)), the rows gathered again
  {
    // XD chunks in flight (the accumulators are dead after the solve)
    constexpr int XD = C::XD;
    f32x4 buf[XD + 1][NTN][2];
#pragma unroll
    for (int s = 0; s < XD && s < NS; ++s) load_chunk(s, buf[s]);
    double xbq = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s + XD < NS) load_chunk(s + XD, buf[(s + XD) % (XD + 1)]);
      f32x4 (&cur)[NTN][2] = buf[s % (XD + 1)];
      float sx[2][4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float v = 0.f;
#pragma unroll
          for (int I = 0; I < NTN; ++I) v += cur[I][h][c] * ul[I];
          sx[h][c] = v;
        }
      // column 32s + 8kk + row16_sum8_column(cl) of x' in the lanes with cl & 2 == 0 (and
      // their neighbours)
      const float sxc = row16_sum8_split(sx, cl);
      if (hasQ) {
        float sb[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float v = 0.f;
#pragma unroll
            for (int I = 0; I < NTN; ++I) v += cur[I][h][c] * cv[I];
            sb[h][c] = v;
          }
        const float sbc = row16_sum8_split(sb, cl);
        xbq += (cl & 2) == 0 ? (double)sxc * (double)sbc : 0.0;
      }
      if ((cl & 2) == 0 && 32 * s + 8 * kk < KP)
        a.X[row * KP + 32 * s + 8 * kk + row16_sum8_column(cl)] = bad ? 0.f : sxc;
      __builtin_amdgcn_sched_barrier(0);
    }
    if (hasQ) xb = wave_sum(xbq);
  }
  double cs = 0.0;
#pragma unroll
  for (int h = 0; h < H; ++h) cs += (double)cwl[h];
  const double csum = wave_sum(cs);
  if (lane == 0) {
    a.rowloss[row] = bad ? 0.0 : csum - xb;  // −λ‖x‖² added after unwhitening
    if (bad && a.status) a.status[row] = 1;
  }
}

// ---------------------------------------------------------------------------------------
// Whitened row kernel, streamed, fp64 (k = 80..128 and 256): the fp32 streamed kernel's plan on the
// fp64 matrix path.  K = Zₛ Zₛᵀ accumulates over 16-column chunks of the gathered rows with
// the next chunk in flight: lane (i, g) holds columns 16s + 4g .. +3 of signal 16I + i, and
// its j-th value is the K index of 16x16x4 f64 MFMA j (exact fp64 products, no split).
// x' = Zₛᵀu gathers the rows a second time after the solve.  Replaces the multi-wave kernel
// whose register-resident Zₛ (half a row of doubles per lane) spilled.
// ---------------------------------------------------------------------------------------
typedef double f64x2 __attribute__((ext_vector_type(2)));

// What the bucket n ≤ 16·NTN is compiled with at KP = 16·NTK.
template <int NTK, int NTN>
struct Wb64Cfg {
  static_assert(NTN >= 1 && NTN <= 5);
  //                                  NTN = 1  2  3  4  5
  // waves per SIMD, by n×n tile count
  static constexpr int WAVES_T[5] = {2, 2, 2, 2, 1};
  // signals per lane (e = lane + 64h)
  static constexpr int H_T[5]     = {1, 1, 1, 1, 2};
  // chunks in flight ahead of the one being consumed in the K pass (beside the NTT
  // accumulator tiles)
  static constexpr int KD_T[5]    = {1, 1, 1, 1, 1};
  // and in the x' pass (after the solve, when the accumulators are dead): 2 since round 6,
  // −0.9 ms per C3 fp64 user half same box, profiles/r06/ab_whiten_lds.txt; round 3 had
  // measured no gain with more chunks kept on chip
  static constexpr int XD_T[5]    = {2, 2, 2, 2, 1};
  // 16-column chunks of Zₛ kept in registers from the K pass to the x' pass (the first KEEP;
  // the rest are gathered again): the registers the n×n Cholesky leaves free at two waves per
  // SIMD (fp64 whitened rows are bound by the fabric's random-row rate, so every chunk not
  // re-gathered is 1/NTK of the second pass's bytes).  NTN ≤ 2: fp64 k = 64 whitened rows on
  // the streamed kernel (round 5: C2 fp64 18.5 -> 17.6 ms/epoch with n ≤ 48 whitened; the
  // register-resident kernel measured slower there)
  static constexpr int KEEP_T[5]  = {6, 6, 2, 1, 0};
  // and the next chunks kept in LDS (the room left under the per-CU LDS at the kernel's waves
  // per SIMD: ≤ 20 KB per row at n ≤ 64, ≤ 40 KB at n ≤ 80)
  static constexpr int KL_T[5]    = {0, 0, 1, 1, 2};
  static constexpr int WAVES = WAVES_T[NTN - 1];
  static constexpr int H = H_T[NTN - 1];
  static constexpr int KD = KD_T[NTN - 1];
  static constexpr int XD = XD_T[NTN - 1];
  static constexpr int KEEP = KEEP_T[NTN - 1] < NTK ? KEEP_T[NTN - 1] : NTK;
  static constexpr int KL = KL_T[NTN - 1] < NTK - KEEP ? KL_T[NTN - 1] : NTK - KEEP;
};
template <int NTK, int NTN, bool TRACE = false>
__global__ __launch_bounds__(64, (Wb64Cfg<NTK, NTN>::WAVES)) void wals_woodbury_st64_kernel(SolveArgs<double> a) {
  using C = Wb64Cfg<NTK, NTN>;
  using M = Mfma<double>;
  using acc_t = typename M::acc_t;
  constexpr int KP = 16 * NTK;
  constexpr int NTT = NTN * (NTN + 1) / 2;
  constexpr int NS = NTK;  // 16-column chunks
  // the diagonal L blocks ride in the panel array (chol.h, LTP): 10.8 KB per row at n ≤ 64
  __shared__ __attribute__((aligned(16))) CholShared<double, NTN, true> S;
  __shared__ __attribute__((aligned(16))) double gq[16 * NTN];
  // Zₛ chunks kept in LDS for the x' pass: [chunk][I·4 + c][lane]
  constexpr int KL = C::KL;
  __shared__ __attribute__((aligned(16))) double kl[KL > 0 ? KL : 1][NTN * 4][64];

  constexpr int H = C::H;  // signals per lane: e = lane + 64h
  const int lane = threadIdx.x;
  const int cl = lane & 15;
  const int kk = lane >> 4;
  uint64_t tr[5] = {0, 0, 0, 0, 0};
  if (TRACE) tr[0] = __builtin_amdgcn_s_memtime();
  const RowDesc dn = a.desc[a.row_begin + blockIdx.x];
  const int64_t row = dn.row;
  const int n = dn.n;  // ≤ 16·NTN by bucketing
  bool mine[H], isP[H], isQ[H];
  int cr[H];
  double wl[H], cwl[H];
  uint64_t mQ[H];
  int bad = 0;
  bool hasQ = false;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const int e = lane + 64 * h;
    mine[h] = e < n;
    cr[h] = mine[h] ? a.col[dn.beg + e] : a.zrow;
    const double vr = mine[h] ? a.val[dn.beg + e] : 0.0;
    wl[h] = mine[h] ? a.alpha * vr : 0.0;
    cwl[h] = mine[h] ? 1.0 + a.alpha * vr : 0.0;
    isP[h] = mine[h] && wl[h] > 0.0;
    isQ[h] = mine[h] && wl[h] == 0.0;
    bad |= __any(mine[h] && wl[h] < 0.0) ? 1 : 0;
    mQ[h] = __ballot(isQ[h]);
    hasQ |= mQ[h] != 0;
  }
  auto bit = [](const uint64_t (&m)[H], int e) -> bool { return (m[e >> 6] >> (e & 63)) & 1; };

  if (TRACE) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    tr[1] = __builtin_amdgcn_s_memtime();
  }
  // this lane's signals 16I + cl (padding signals read the all-zero row a.zrow)
  const f64x2* zp[NTN];
#pragma unroll
  for (int I = 0; I < NTN; ++I) {
    const int ce = __shfl(cr[I >> 2], (16 * I + cl) & 63, 64);
    zp[I] = reinterpret_cast<const f64x2*>(a.Y + (uint64_t)(uint32_t)ce * KP);
  }
  auto load_chunk = [&](int s, double (&buf)[NTN][4]) {
    const int c2 = 8 * s + 2 * kk;  // f64x2 index of column 16s + 4kk
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const f64x2 u = zp[I][c2], v = zp[I][c2 + 1];
      buf[I][0] = u[0], buf[I][1] = u[1], buf[I][2] = v[0], buf[I][3] = v[1];
    }
  };

  acc_t acc[NTT];
#pragma unroll
  for (int t = 0; t < NTT; ++t) acc[t] = acc_t{0.0, 0.0, 0.0, 0.0};
  double sq[NTN];  // z_eᵀ Σ_{f∈Q} z_f over this lane's columns (rows with Q signals)
#pragma unroll
  for (int I = 0; I < NTN; ++I) sq[I] = 0.0;
  constexpr int KEEP = C::KEEP;
  double keep[KEEP > 0 ? KEEP : 1][NTN][4];
  {
    // a ring of KD + 1 chunk buffers: chunk s + KD is in flight while chunk s is consumed
    // (the loop unrolls fully, so every ring index is a compile-time constant)
    constexpr int KD = C::KD;
    double buf[KD + 1][NTN][4];
#pragma unroll
    for (int s = 0; s < KD && s < NS; ++s) load_chunk(s, buf[s]);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s + KD < NS) load_chunk(s + KD, buf[(s + KD) % (KD + 1)]);
      double (&cur)[NTN][4] = buf[s % (KD + 1)];
      if (s < KEEP) {
#pragma unroll
        for (int I = 0; I < NTN; ++I)
#pragma unroll
          for (int c = 0; c < 4; ++c) keep[s < KEEP ? s : 0][I][c] = cur[I][c];
      } else if (s < KEEP + KL) {
#pragma unroll
        for (int I = 0; I < NTN; ++I)
#pragma unroll
          for (int c = 0; c < 4; ++c) kl[s - KEEP < KL ? s - KEEP : 0][4 * I + c][lane] = cur[I][c];
      }
      if (hasQ) {
        double g[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double v = 0.0;
#pragma unroll
          for (int I = 0; I < NTN; ++I)
            if (bit(mQ, 16 * I + cl)) v += cur[I][c];
          g[c] = v;
        }
        row16_sum4(g);
#pragma unroll
        for (int I = 0; I < NTN; ++I)
#pragma unroll
          for (int c = 0; c < 4; ++c) sq[I] += cur[I][c] * g[c];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int I = 0; I < NTN; ++I) {
#pragma unroll
          for (int J = 0; J <= I; ++J) {
            const int t = tile_index(I, J);
            acc[t] = M::mma(cur[I][j], cur[J][j], acc[t]);
          }
        }
      }
      // one chunk and the next chunks' loads live at a time
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  double xb = 0.0;
  double ul[NTN], cv[NTN];
  // the n×n system: one factorization for both forms (a copy per form pushed the n = 64
  // instance past three waves' registers)
  double iw[H], rhs[H];
  uint64_t mP[H];
#pragma unroll
  for (int h = 0; h < H; ++h) mP[h] = __ballot(isP[h]);
  if (!hasQ) {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      iw[h] = isP[h] ? 1.0 / wl[h] : 1.0;
      rhs[h] = isP[h] ? cwl[h] * iw[h] : 0.0;
    }
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const double iwd = __shfl(iw[I >> 2], (16 * I + cl) & 63, 64);
      const int t = tile_index(I, I);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] += M::crow(lane, r) == cl ? iwd : 0.0;
    }
  } else {
    // Q signals (w = 0): u_Q = 1 moves to the right-hand side, the Q rows/columns become
    // identity
#pragma unroll
    for (int h = 0; h < H; ++h) rhs[h] = isP[h] ? cwl[h] / wl[h] : 0.0;
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      double v = sq[I];
      v += shfl_xor(v, 16);
      v += shfl_xor(v, 32);
      if (kk == 0) gq[16 * I + cl] = v;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const double kqv = lane + 64 * h < 16 * NTN ? gq[lane + 64 * h] : 0.0;
      if (isP[h]) rhs[h] -= kqv;
      iw[h] = isP[h] ? 1.0 / wl[h] : 0.0;
    }
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const double iwd = __shfl(iw[I >> 2], (16 * I + cl) & 63, 64);
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        const int t = tile_index(I, J);
        const int f = 16 * J + cl;
        const bool pf = bit(mP, f);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = 16 * I + M::crow(lane, r);
          const bool pe = bit(mP, e);
          double v = acc[t][r];
          if (pe && pf) v += (e == f) ? iwd : 0.0;
          else v = (e == f) ? 1.0 : 0.0;
          acc[t][r] = v;
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < H; ++h)
    if (lane + 64 * h < 16 * NTN) S.bw[lane + 64 * h] = rhs[h];
  __syncthreads();
  if (TRACE) tr[2] = __builtin_amdgcn_s_memtime();
  row_chol<double, NTN>(acc, S, lane, bad);
  if (TRACE) tr[3] = __builtin_amdgcn_s_memtime();
  if (!hasQ) {
    double xbl = 0.0;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const double ue = lane + 64 * h < 16 * NTN ? S.xs[lane + 64 * h] : 0.0;
      xbl += isP[h] ? rhs[h] * (cwl[h] - ue) : 0.0;
    }
    xb = wave_sum(xbl);
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      ul[I] = S.xs[16 * I + cl];
      cv[I] = 0.0;
    }
  } else {
#pragma unroll
    for (int I = 0; I < NTN; ++I) {
      const int e = 16 * I + cl;
      const bool pe = bit(mP, e);
      const bool qe = bit(mQ, e);
      ul[I] = pe ? S.xs[e] : (qe ? 1.0 : 0.0);
      cv[I] = __shfl(cwl[I >> 2], e & 63, 64);
    }
  }

  // x' = Zₛᵀu (and for rows with Q signals xᵀb = x'ᵀ(Zₛᵀc)), the rows gathered again
  {
    // XD chunks in flight: the Gram's accumulators are dead here, so the x' pass can hold
    // a deeper ring than the K pass (each chunk costs little compute: its loads would
    // otherwise be waited for one after the other)
    constexpr int XD = C::XD;
    constexpr int KT = KEEP + KL;  // chunks kept on chip (registers, then LDS)
    constexpr int NG = NS - KT;    // chunks gathered again
    double buf[XD + 1][NTN][4];
#pragma unroll
    for (int q = 0; q < XD && q < NG; ++q) load_chunk(KT + q, buf[q]);
    double xbq = 0.0;
    auto xchunk = [&](int s, const double (&cur)[NTN][4]) {
      double sx[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double v = 0.0;
#pragma unroll
        for (int I = 0; I < NTN; ++I) v += cur[I][c] * ul[I];
        sx[c] = v;
      }
      // column 16s + 4kk + (cl >> 2) of x' in lanes cl = 0, 4, 8, 12 (and their neighbours)
      const double sxc = row16_sum4_split(sx, cl);
      if (hasQ) {
        double sb[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double v = 0.0;
#pragma unroll
          for (int I = 0; I < NTN; ++I) v += cur[I][c] * cv[I];
          sb[c] = v;
        }
        const double sbc = row16_sum4_split(sb, cl);
        xbq += (cl & 3) == 0 ? sxc * sbc : 0.0;
      }
      if ((cl & 3) == 0) a.X[row * KP + 16 * s + 4 * kk + (cl >> 2)] = bad ? 0.0 : sxc;
      __builtin_amdgcn_sched_barrier(0);
    };
    // the kept chunks while the first gathers are in flight, then the gathered ring
#pragma unroll
    for (int s = 0; s < KEEP; ++s) xchunk(s, keep[s]);
#pragma unroll
    for (int s = 0; s < KL; ++s) {
      double cur[NTN][4];
#pragma unroll
      for (int I = 0; I < NTN; ++I)
#pragma unroll
        for (int c = 0; c < 4; ++c) cur[I][c] = kl[s][4 * I + c][lane];
      xchunk(KEEP + s, cur);
    }
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      if (q + XD < NG) load_chunk(KT + q + XD, buf[(q + XD) % (XD + 1)]);
      xchunk(KT + q, buf[q % (XD + 1)]);
    }
    if (hasQ) xb = wave_sum(xbq);
  }
  double cs = 0.0;
#pragma unroll
  for (int h = 0; h < H; ++h) cs += cwl[h];
  const double csum = wave_sum(cs);
  if (lane == 0) {
    a.rowloss[row] = bad ? 0.0 : csum - xb;  // −λ‖x‖² added after unwhitening
    if (bad && a.status) a.status[row] = 1;
  }
  if (TRACE && lane == 0) {
    tr[4] = __builtin_amdgcn_s_memtime();
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    uint64_t* o = a.trace + 8 * (a.row_begin + blockIdx.x);
#pragma unroll
    for (int j = 0; j < 5; ++j) o[j] = tr[j];
    o[5] = hw | ((uint64_t)xcc << 32);
    o[6] = (uint64_t)n;
    o[7] = (uint64_t)row;
  }
}

#ifndef QMFX_KERNELS_ONLY
// f(integral_constant<int, ntn>) for 1 ≤ ntn ≤ MAX: the buckets wb_max_ntn gives a tiling are
// the only ones instantiated
template <int MAX, typename F>
static hipError_t dispatch_ntn(int ntn, F&& f) {
  if constexpr (MAX >= 1) {
    if (ntn == MAX) return f(std::integral_constant<int, MAX>{});
    return dispatch_ntn<MAX - 1>(ntn, f);
  } else {
    return hipErrorInvalidValue;
  }
}

// fp32: the streamed kernel at every tiling
template <int NTK>
static hipError_t launch_woodbury_f32_ntk(const SolveArgs<float>& a, int ntn, hipStream_t s) {
  if (a.nrows <= 0) return hipSuccess;
  if (!a.desc) return hipErrorInvalidValue;
  return dispatch_ntn<wb_max_ntn(4, NTK)>(ntn, [&](auto N) {
    return launch_row_chunks(a, 64, [&](const SolveArgs<float>& c) {
      hipLaunchKernelGGL((wals_woodbury_st_kernel<NTK, decltype(N)::value>),
                         dim3((unsigned)c.nrows), dim3(64), 0, s, c);
    });
  });
}

// fp64: k ≤ 48 on the register-resident kernel, k = 64 .. 128 and 256 on the streamed one
template <int NTK>
static hipError_t launch_woodbury_f64_ntk(const SolveArgs<double>& a, int ntn, hipStream_t s) {
  if (a.nrows <= 0) return hipSuccess;
  if (!a.desc) return hipErrorInvalidValue;
  return dispatch_ntn<wb_max_ntn(8, NTK)>(ntn, [&](auto N) {
    constexpr int NTN = decltype(N)::value;
    return launch_row_chunks(a, 64, [&](const SolveArgs<double>& c) {
      const dim3 grid((unsigned)c.nrows), b(64);
      if constexpr (NTK < 4) {
        if (c.trace)
          hipLaunchKernelGGL((wals_woodbury_kernel<NTK, NTN, true>), grid, b, 0, s, c);
        else
          hipLaunchKernelGGL((wals_woodbury_kernel<NTK, NTN, false>), grid, b, 0, s, c);
      } else {
        if (c.trace)
          hipLaunchKernelGGL((wals_woodbury_st64_kernel<NTK, NTN, true>), grid, b, 0, s, c);
        else
          hipLaunchKernelGGL((wals_woodbury_st64_kernel<NTK, NTN>), grid, b, 0, s, c);
      }
    });
  });
}

hipError_t launch_wals_woodbury(const SolveArgs<float>& a, int nt, int ntn, hipStream_t s) {
  return dispatch_nt_w(
      nt, [&](auto N) { return launch_woodbury_f32_ntk<decltype(N)::value>(a, ntn, s); });
}
hipError_t launch_wals_woodbury(const SolveArgs<double>& a, int nt, int ntn, hipStream_t s) {
  return dispatch_nt_w(
      nt, [&](auto N) { return launch_woodbury_f64_ntk<decltype(N)::value>(a, ntn, s); });
}
#endif  // QMFX_KERNELS_ONLY

}  // namespace qmfx
