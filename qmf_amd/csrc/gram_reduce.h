// Fixed-order sum of the YᵀY partials, shared by the one-wave (wals.hip) and the tiled
// (gram_big.hip) YᵀY.
#pragma once
#include "common.h"

namespace qmfx {

// Fixed-order sum of the partials: 16 outputs per 256-thread block, each summed as 16
// consecutive chunks of blocks (thread (chunk, output)), then the chunk sums in order —
// deterministic, and 16× the parallelism of one thread per output (C2: 0.32 → ~0.03 ms).
__device__ __forceinline__ double gram_reduce_one(const double* partial, int nblocks,
                                                  int64_t stride, int off, double (*red)[16],
                                                  int o, int ch) {
  const int cs = (nblocks + 15) / 16;
  const int b0 = ch * cs, b1 = b0 + cs < nblocks ? b0 + cs : nblocks;
  double s = 0.0;
  for (int b = b0; b < b1; ++b) s += partial[(int64_t)b * stride + off];
  red[ch][o] = s;
  __syncthreads();
  double t = 0.0;
  if (ch == 0)
    for (int c = 0; c < 16; ++c) t += red[c][o];
  return t;
}

}  // namespace qmfx
