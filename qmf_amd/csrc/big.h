// The multi-wave tilings (k > 128 rows, wals_big.hip; tiled YᵀY, gram_big.hip): one workgroup
// of NW waves shares the NT(NT+1)/2 lower 16×16 tiles of a k×k matrix.  The configuration of
// a tiling, the tile → wave map and the LDS-staged Gram step both units use.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

// `#pragma unroll 2` on the Gram step loops is not honoured for every tiling (those keep a
// rolled loop); dropping the hint costs the fp32 NT = 16 kernels 24-44 VGPRs, so it stays
#pragma clang diagnostic ignored "-Wpass-failed"
#include "kernels.h"
#include "rowsolve.h"

namespace qmfx {

template <typename T, int NT>
struct BigCfg {
  static constexpr int KP = 16 * NT;
  static constexpr int NTT = NT * (NT + 1) / 2;
  // waves per row: ≤ 17 fp32 / ≤ 10 fp64 accumulator tiles per wave (fp64 NT ≤ 8: the tiled
  // YᵀY only; those rows run the one-wave direct kernel)
  static constexpr int NW = sizeof(T) == 4 ? (NT <= 10 ? 4 : 8) : (NT <= 8 ? 4 : 8);
  // split-bf16 Gram (fp32 k = 256, where NT = 2·NW): the loader threads split each staged
  // element once into bf16 hi/mid/lo planes ([column][signal], 32 signals = one 16x16x32 MFMA
  // K step) and wave W owns block rows W and NT−1−W (NT + 1 tiles), reading each column
  // block's planes once per stage for both rows
  static constexpr bool SPLIT = sizeof(T) == 4 && NT == 16;
  // fp64: every wave gathers its own operand fragments of the row's signals (big_gram_stream),
  // with no LDS staging and no barrier in the Gram
  static constexpr bool STREAM = sizeof(T) == 8;
  // row-pair tile map (wave W owns block rows W and NT−1−W: NT + 1 tiles)
  static constexpr bool PAIR = SPLIT || (STREAM && NT == 2 * NW);
  // one wave-specialised copy of the row solve per wave (compile-time tile map) and the LDLᵀ
  // factorization (big_ldl_solve, two panel buffers in turn): the streamed fp64 rows and the
  // split fp32 rows.  The other rows (fp32 below k = 256): the LDS-staged Gram with a runtime
  // tile map and the readlane Cholesky (big_panel_all)
  static constexpr bool WSPEC = STREAM || SPLIT;
  // waves per SIMD the row kernel is compiled for (512-thread workgroups: two)
  static constexpr int WPE = (64 * NW + 255) / 256;
  static constexpr int TPW = PAIR ? NT + 1 : (NTT + NW - 1) / NW;
  static constexpr int SPAD = 40;  // bf16 per plane column (32 signals + 16 B pad: no bank conflicts)
  static constexpr int NTHR = 64 * NW;
  static constexpr int SIG = sizeof(T) == 4 ? 32 : 16;  // signals per LDS stage
  // split Gram: signal quads per stage = loader threads per column group, each with its own
  // partial of b and Σc (every tiling keeps the slots: one LDS layout)
  static constexpr int NQ = 8;
  static constexpr int VEC = 16 / sizeof(T);             // elements per 16-B load
  static constexpr int CPR = KP / VEC;                   // 16-B chunks per row
  static constexpr int TRIPS = (SIG * CPR + NTHR - 1) / NTHR;
  // padded LDS row of a panel (fp32: 16-B aligned rows for the b128 row accesses)
  static constexpr int PLD = sizeof(T) == 4 ? 20 : 17;
  // LDS fragments reused across a wave's tiles in the staged Gram (big_gram_step, tile map at
  // compile time); the fp64 tilings above NT = 11 lack the registers for it (the tiled YᵀY
  // only: the fp64 rows stream)
  static constexpr bool REUSE = sizeof(T) == 4 || NT <= 11;
};

// tile s of wave W: round-robin t = W + NW·s, or (split map) rows W and NT−1−W
template <typename C>
__host__ __device__ constexpr void big_tile(int W, int s, int& I, int& J) {
  if constexpr (C::PAIR) {
    constexpr int NT = C::KP / 16;
    if (s <= W) {
      I = W;
      J = s;
    } else {
      I = NT - 1 - W;
      J = s - W - 1;
    }
  } else {
    const int t = W + C::NW * s;
    if (t < C::NTT) {
      int i = 0;
      while ((i + 1) * (i + 2) / 2 <= t) ++i;
      I = i;
      J = t - i * (i + 1) / 2;
    } else {
      I = J = -1;
    }
  }
}

// Calls f(integral_constant<W>) for the wave-uniform wave index wv (compile-time tile maps).
template <int NW, int W = 0, typename F>
__device__ __forceinline__ void dispatch_wave(int wv, F&& f) {
  if constexpr (W < NW) {
    if (wv == W)
      f(std::integral_constant<int, W>{});
    else
      dispatch_wave<NW, W + 1>(wv, f);
  }
}

// One 4-signal step of the Gram for the tiles of wave W (t = W + NW·s, compile-time map):
// the wave reads each 16-row fragment of the staged signals once (NT LDS reads instead of
// two per tile) and reuses it for every tile in its tile row or column.
template <typename T, int NT, int W>
__device__ __forceinline__ void big_gram_step(typename Mfma<T>::acc_t* acc, const T* yk, T wk) {
  using C = BigCfg<T, NT>;
  using M = Mfma<T>;
  T y[NT], wy[NT];
#pragma unroll
  for (int J = 0; J < NT; ++J) {
    y[J] = yk[16 * J];
    wy[J] = wk * y[J];
  }
#pragma unroll
  for (int s = 0; s < C::TPW; ++s) {
    int I = -1, J = -1;
    big_tile<C>(W, s, I, J);
    if (I >= 0) acc[s] = M::mma(y[I], wy[J], acc[s]);
  }
}

}  // namespace qmfx
