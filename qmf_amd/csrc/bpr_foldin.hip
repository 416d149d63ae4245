// BPR fold-in on MI355X: SGD on a new user's row alone, item factors and biases frozen.
//
// Reference (taozhijiang/qmf): the user line of BPREngine::update (qmf/bpr/BPREngine.cpp:178-220),
// which reads the old item rows; the schedule of BPREngine::optimize (:146-176).
//
// One wave64 owns one new row for the whole schedule: lanes hold factor elements (KP ≤ 64·E) and
// the row stays in registers from its start value to its single store.  Nothing another wave
// reads is written, so the item rows and biases come through plain loads (the epoch kernel's
// agent-scope atomics are for rows that change under it), there are no atomics, and a row's
// result depends on nothing but its own positives, the seed and the items: it is the same in
// every launch, whatever the grid.  The negatives are the epoch kernel's counter-based draws
// (bpr_common.h), keyed by pass and by the positive's position in the call's CSR.
#include "bpr_common.h"
#include "kernels.h"

namespace qmfx {

namespace {

template <typename T, int E>
__device__ __forceinline__ void load_frozen(Row<T, E>& r, const T* base, int lane, int kp) {
#pragma unroll
  for (int e = 0; e < E; ++e) r.v[e] = (lane + 64 * e < kp) ? base[lane + 64 * e] : T(0);
}

// Positive i of pass e: its num_neg steps (p, q_{c_i}, q_n), four negatives at a time.  The
// draws of a group come first and their rows are loaded together, then the steps run in draw
// order on the row in registers.  The next positive's row (qp_next, of the next pass's first
// positive after the last) is requested before the group's draws, so it arrives behind them.
template <typename T, int E>
__global__ __launch_bounds__(64) void bpr_fold_kernel(BprFoldArgs<T> a) {
  const int lane = threadIdx.x;
  const int kp = a.kp;
  const uint64_t seed_key = mix64(a.seed ^ 0xb5ad4eceda1ce2a9ull);
  bool ok = true;
  for (int64_t r = blockIdx.x; r < a.nrows; r += gridDim.x) {
    const int64_t rb = a.rowptr[r], cnt = a.rowptr[r + 1] - rb;
    if (cnt == 0) {  // keeps its start value
      if (lane == 0) a.losses[r] = 0.0;
      continue;
    }
    const int32_t* items = a.col + rb;
    // the rejection set of the draws: up to 64 positives, one per lane
    int32_t mine = items[lane < cnt ? lane : 0];
    mine = lane < cnt ? mine : -1;
    Row<T, E> p, qp_next;
    load_frozen(p, a.X + r * kp, lane, kp);
    int64_t c_next = items[0];
    load_frozen(qp_next, a.I + c_next * kp, lane, kp);
    T bp_next = a.bias ? a.bias[c_next] : T(0);
    double loss = 0.0;
    for (int e = 0; e < a.nepochs; ++e) {
      const T lr = a.lr[e];
      const bool last = e == a.nepochs - 1;
      const uint64_t pass_key = mix64(seed_key ^ (uint64_t)e);
      for (int64_t i = 0; i < cnt; ++i) {
        const Row<T, E> qp = qp_next;
        const T bp = bp_next;
        c_next = items[i + 1 < cnt ? i + 1 : 0];
        load_frozen(qp_next, a.I + c_next * kp, lane, kp);
        if (a.bias) bp_next = a.bias[c_next];
        const uint64_t pkey = mix64(pass_key ^ (uint64_t)(rb + i));
        const uint32_t fk = (uint32_t)pkey ^ (uint32_t)(pkey >> 32);
        for (int j0 = 0; j0 < a.num_neg; j0 += 4) {
          const int nn = a.num_neg - j0 < 4 ? a.num_neg - j0 : 4;
          int64_t n[4] = {0, 0, 0, 0};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < nn)
              n[j] = draw_negative_t(a, items, cnt, mine, fk, 4099u * (uint32_t)(j0 + j), lane);
          Row<T, E> qn[4];
          T bn[4] = {T(0), T(0), T(0), T(0)};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < nn) {
              load_frozen(qn[j], a.I + n[j] * kp, lane, kp);
              if (a.bias) bn[j] = a.bias[n[j]];
            }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j >= nn) break;
            T part = T(0);
#pragma unroll
            for (int f = 0; f < E; ++f) part += p.v[f] * (qp.v[f] - qn[j].v[f]);
            T x = wave_total(part);
            if (a.bias) x += bp - bn[j];
            const T eg = neg_sigmoid(x);
            if (!isfinite(eg)) {
              ok = false;
              continue;  // the reference aborts (CHECK); the row is left as it was
            }
            if (last) loss += log(1.0 + exp(-(double)x));
#pragma unroll
            for (int f = 0; f < E; ++f)
              p.v[f] = p.v[f] + lr * (eg * (qp.v[f] - qn[j].v[f]) - a.user_lambda * p.v[f]);
          }
        }
      }
    }
#pragma unroll
    for (int f = 0; f < E; ++f)
      if (lane + 64 * f < kp) a.X[r * kp + lane + 64 * f] = p.v[f];
    if (lane == 0) a.losses[r] = loss;
  }
  if (!ok && lane == 0) *a.bad = 1;
}

template <typename T, int E>
hipError_t bpr_fold(const BprFoldArgs<T>& a, hipStream_t s) {
  hipLaunchKernelGGL((bpr_fold_kernel<T, E>), dim3(a.grid), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace

// One workgroup per row, so that rows of any length spread over the chip as workgroups
// retire; past 2^20 rows the waves stride.
int bpr_fold_grid(int64_t nrows) {
  int64_t cap = (int64_t)1 << 20;
  if (const char* e = std::getenv("QMFX_BPR_FOLD_GRID"))
    if (std::atoll(e) > 0 && std::atoll(e) < cap) cap = std::atoll(e);
  return (int)(nrows < cap ? nrows : cap);
}

hipError_t launch_bpr_fold(const BprFoldArgs<float>& a, hipStream_t s) {
#define CALL(E) bpr_fold<float, E>(a, s)
  QMFX_E_SWITCH(a.kp, CALL)
#undef CALL
}
hipError_t launch_bpr_fold(const BprFoldArgs<double>& a, hipStream_t s) {
#define CALL(E) bpr_fold<double, E>(a, s)
  QMFX_E_SWITCH(a.kp, CALL)
#undef CALL
}

}  // namespace qmfx
