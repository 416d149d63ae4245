// Explanations: why is target t in row r's list?  With A = G + Σ αv·yyᵀ + λI the score of the
// row solved from its own signals is y_tᵀA⁻¹b = Σ_e (1 + αv_e)·y_eᵀA⁻¹y_t (Hu, Koren, Volinsky
// 2008, §5): every signal of the row contributes an additive share.
//
// One 256-thread workgroup takes one query (a row and its targets) at a time:
//   1. A is assembled in fp64 by build_system (system.h), as a packed lower triangle;
//   2. A = LLᵀ in place, right-looking, one column per step: the scaled column is copied to a
//      contiguous LDS vector, so the trailing update reads no column of the packed triangle;
//   3. per block of kExplainRhs targets: forward and back substitution for all of them at
//      once (thread = (target, one of 32 row lanes)), giving z_t = A⁻¹y_t;
//   4. the row's signals are staged 16 at a time through LDS again; contribution
//      c_e·(y_e·z_t), the sum of a dot product in factor order; written to the full vector,
//      added to the total in CSR order and inserted into the target's top-M list.
// The triangle lives in LDS up to KP = 128 (66 KB) and in a per-workgroup global scratch
// above (KP = 256: 263 KB, L2-resident); everything else is LDS in both forms.  Only the
// leading k×k block is factored: the padding rows of A are the identity.
#include <float.h>

#include "common.h"
#include "kernels.h"
#include "system.h"

namespace qmfx {

namespace {

constexpr int NB = kExplainRhs;
constexpr int EX_LANES = FB_THREADS / NB;  // row lanes per right-hand side
constexpr int EX_MAX_GRID_LDS = 1024;
constexpr int EX_MAX_GRID_SCRATCH = 256;
static_assert(NB == 8 && FB_CHUNK * NB <= FB_THREADS, "thread = (signal of the chunk, target)");

// dynamic LDS of one workgroup, in bytes (the kernel carves it in this order)
size_t explain_lds_bytes(int kp, int topm, bool in_lds) {
  const size_t ld = in_lds ? kExplainLdsMaxKP : 256;
  size_t d = in_lds ? (size_t)kp * (kp + 1) / 2 : 0;  // the packed factor
  d += 2 * (size_t)kp;                                // b, the current column
  d += FB_CHUNK * ld + 2 * FB_CHUNK;                  // staged signals, their w and c
  d += 2 * (size_t)kp * NB;                           // right-hand sides: R and W
  d += FB_CHUNK * NB + NB;                            // a chunk's contributions, (unused) pad
  d += (size_t)NB * topm;                             // top-M values
  return d * sizeof(double) + (size_t)NB * topm * sizeof(int);  // … and positions
}

template <typename T, bool IN_LDS>
__global__ __launch_bounds__(FB_THREADS) void explain_kernel(ExplainArgs<T> a) {
  extern __shared__ double smem[];
  constexpr int LD = IN_LDS ? kExplainLdsMaxKP : 256;
  const int tid = threadIdx.x;
  const int KP = a.sys.kp, k = a.sys.k, M = a.topm;
  const size_t tri = (size_t)KP * (KP + 1) / 2;
  double* p = smem;
  double* L;
  if constexpr (IN_LDS) {
    L = p;
    p += tri;
  } else {
    L = a.sys.scratch + (size_t)blockIdx.x * tri;
  }
  double* bvec = p;
  double* colj = bvec + KP;
  double(*ys)[LD] = reinterpret_cast<double(*)[LD]>(colj + KP);
  double* ws = colj + KP + FB_CHUNK * LD;
  double* cs = ws + FB_CHUNK;
  double* R = cs + FB_CHUNK;
  double* W = R + (size_t)KP * NB;
  double* cbuf = W + (size_t)KP * NB;
  double* topv = cbuf + FB_CHUNK * NB + NB;
  int* topp = reinterpret_cast<int*>(topv + (size_t)NB * M);
  const int r = tid % NB, lane = tid / NB;  // solves: right-hand side and row lane
  const T* Y = a.sys.Y;

  for (int64_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
    const int64_t t0 = a.qptr[q], t1 = a.qptr[q + 1];
    if (t0 >= t1) continue;
    const int64_t row = a.rows ? a.rows[q] : q;
    const int64_t beg = a.rowptr[row], end = a.rowptr[row + 1], n = end - beg;
    __syncthreads();  // the previous query's readers of the LDS arrays are done
    double csum = 0.0;
    build_system<T, LD, true>(a.sys, beg, end, L, bvec, csum, ys, ws, cs, tid);

    // A = LLᵀ.  Every thread reads the same pivot, so the exit is uniform.
    bool spd = true;
    for (int j = 0; j < k; ++j) {
      const size_t jj = (size_t)j * (j + 1) / 2 + j;
      const double d = L[jj];
      if (!(d > 0.0) || !(d <= DBL_MAX)) {
        spd = false;
        break;
      }
      const double s = sqrt(d);
      for (int i = j + 1 + tid; i < k; i += FB_THREADS) {
        const size_t ij = (size_t)i * (i + 1) / 2 + j;
        const double v = L[ij] / s;
        L[ij] = v;
        colj[i] = v;
      }
      __syncthreads();
      if (tid == 0) L[jj] = s;
      const int ty = tid >> 4, tx = tid & 15;
      for (int i = j + 1 + ty; i < k; i += 16) {
        const double li = colj[i];
        double* Li = L + (size_t)i * (i + 1) / 2;
        for (int c = j + 1 + tx; c <= i; c += 16) Li[c] -= li * colj[c];
      }
      __syncthreads();
    }
    if (!spd) {
      if (tid == 0) atomicMin(a.first_bad, (unsigned long long)q);
      continue;
    }

    const int64_t all0 = a.all ? a.allq[q] : 0;
    for (int64_t tb = t0; tb < t1; tb += NB) {
      const int nb = (int)(t1 - tb < NB ? t1 - tb : NB);
      // right-hand sides y_t, widened; R[i·NB + r]
      for (int idx = tid; idx < k * NB; idx += FB_THREADS) {
        const int i = idx / NB, rr = idx % NB;
        R[idx] = rr < nb ? (double)Y[(size_t)a.targets[tb + rr] * KP + i] : 0.0;
      }
      __syncthreads();
      // L w = y, column by column: w_j is final once columns < j are applied
      for (int j = 0; j < k; ++j) {
        const size_t jj = (size_t)j * (j + 1) / 2 + j;
        const double wj = R[j * NB + r] / L[jj];
        if (lane == 0) W[j * NB + r] = wj;
        for (int i = j + 1 + lane; i < k; i += EX_LANES)
          R[i * NB + r] -= L[(size_t)i * (i + 1) / 2 + j] * wj;
        __syncthreads();
      }
      // Lᵀ z = w, from the last row up; z overwrites R
      for (int j = k - 1; j >= 0; --j) {
        const double* Lj = L + (size_t)j * (j + 1) / 2;
        const double zj = W[j * NB + r] / Lj[j];
        if (lane == 0) R[j * NB + r] = zj;
        for (int i = lane; i < j; i += EX_LANES) W[i * NB + r] -= Lj[i] * zj;
        __syncthreads();
      }
      // contributions, the signals staged FB_CHUNK at a time
      double tot = 0.0;
      int cnt = 0;
      for (int64_t base = beg; base < end; base += FB_CHUNK) {
        const int m = (int)(end - base < FB_CHUNK ? end - base : FB_CHUNK);
        {
          const int e = tid >> 4;
          const size_t yrow = e < m ? (size_t)(uint32_t)a.sys.col[base + e] * KP : 0;
          for (int f = tid & 15; f < k; f += 16) ys[e][f] = e < m ? (double)Y[yrow + f] : 0.0;
        }
        if (tid < FB_CHUNK)
          cs[tid] = tid < m ? 1.0 + (double)a.sys.alpha * (double)a.sys.val[base + tid] : 0.0;
        __syncthreads();
        if (tid < FB_CHUNK * NB) {
          const int e = tid / NB;
          double s = 0.0;
          for (int f = 0; f < k; ++f) s += ys[e][f] * R[f * NB + r];
          const double v = cs[e] * s;
          cbuf[e * NB + r] = v;
          if (a.all && e < m && r < nb)
            a.all[all0 + (tb + r - t0) * n + (base - beg) + e] = v;
        }
        __syncthreads();
        if (tid < nb) {
          double* tv = topv + (size_t)tid * M;
          int* tp = topp + (size_t)tid * M;
          for (int e = 0; e < m; ++e) {
            const double v = cbuf[e * NB + tid];
            tot += v;
            // after every entry that is ≥ v: an equal contribution ranks by position
            if (cnt < M || v > tv[M - 1]) {
              int at = cnt < M ? cnt : M - 1;
              while (at > 0 && tv[at - 1] < v) {
                tv[at] = tv[at - 1];
                tp[at] = tp[at - 1];
                --at;
              }
              tv[at] = v;
              tp[at] = (int)(base - beg) + e;
              if (cnt < M) ++cnt;
            }
          }
        }
        __syncthreads();
      }
      if (tid < nb) {
        const int64_t pair = tb + tid;
        const double* tv = topv + (size_t)tid * M;
        const int* tp = topp + (size_t)tid * M;
        a.totals[pair] = tot;
        a.counts[pair] = cnt;
        for (int s = 0; s < M; ++s) {
          const bool in = s < cnt;
          a.sources[pair * M + s] = in ? (int64_t)a.sys.col[beg + tp[s]] : -1;
          a.positions[pair * M + s] = in ? (int64_t)tp[s] : -1;
          a.contribs[pair * M + s] = in ? tv[s] : 0.0;
        }
      }
      __syncthreads();
    }
  }
}

template <typename T>
hipError_t explain(const ExplainArgs<T>& a, hipStream_t s) {
  if (a.nq <= 0) return hipSuccess;
  if (a.sys.kp > 256 || a.topm < 1 || a.topm > kRecMaxN) return hipErrorInvalidValue;
  const bool in_lds = a.sys.kp <= kExplainLdsMaxKP;
  const size_t lds = explain_lds_bytes(a.sys.kp, a.topm, in_lds);
  const void* fn = in_lds ? (const void*)explain_kernel<T, true> : (const void*)explain_kernel<T, false>;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const dim3 grid(explain_grid(a.nq, a.sys.kp)), block(FB_THREADS);
  if (in_lds)
    hipLaunchKernelGGL((explain_kernel<T, true>), grid, block, lds, s, a);
  else
    hipLaunchKernelGGL((explain_kernel<T, false>), grid, block, lds, s, a);
  return hipGetLastError();
}

}  // namespace

// Workgroups loop over the queries, so the scratch of the KP > 128 form is bounded.
int explain_grid(int64_t nq, int kp) {
  const int64_t cap = kp <= kExplainLdsMaxKP ? EX_MAX_GRID_LDS : EX_MAX_GRID_SCRATCH;
  return (int)(nq < 1 ? 1 : (nq > cap ? cap : nq));
}

hipError_t launch_explain(const ExplainArgs<float>& a, hipStream_t s) { return explain(a, s); }
hipError_t launch_explain(const ExplainArgs<double>& a, hipStream_t s) { return explain(a, s); }

}  // namespace qmfx
