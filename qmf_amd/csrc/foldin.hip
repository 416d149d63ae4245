// Fold-in: the row plan of a foreign CSR on the device, and the gather of the solved rows.
//
// build_buckets (api_signals.cpp) walks a side's rowptr on the host and stable_sorts the
// direct rows; for rows that arrive with a call that walk would sit on the critical path.
// Here a kernel turns every row into one 64-bit key (kernels.h FoldKeyBits), one radix sort
// (data.hip sort_keys) orders them, and a second kernel expands the sorted keys into the order
// list, the per-slot descriptors and the nine bucket boundaries.  The boundaries need neither
// a scan nor an atomic: in sorted order the slot where the class changes writes the first slot
// of every class it enters, so each boundary has exactly one writer.
#include "common.h"
#include "kernels.h"

namespace qmfx {

namespace {

constexpr int FI_THREADS = 256;

inline unsigned fi_blocks(int64_t n) { return (unsigned)((n + FI_THREADS - 1) / FI_THREADS); }

int bit_width(uint64_t x) {
  int b = 0;
  while (x) {
    ++b;
    x >>= 1;
  }
  return b;
}

// class of a sorted key: 0 .. kMaxNTN − 1 whitened bucket, kMaxNTN direct
__device__ inline int fold_class(uint64_t key, FoldKeyBits kb) {
  if (key >> (kb.row_bits + kb.n_bits)) return kMaxNTN;
  return (int)(key >> kb.row_bits);
}

__global__ __launch_bounds__(FI_THREADS) void fold_keys_kernel(const int64_t* rowptr,
                                                               int64_t nrows, int max_ntn,
                                                               int64_t max_n, FoldKeyBits kb,
                                                               uint64_t* keys) {
  const int64_t r = (int64_t)blockIdx.x * FI_THREADS + threadIdx.x;
  if (r >= nrows) return;
  const int64_t n = rowptr[r + 1] - rowptr[r];
  const int64_t ntn = ((n > 1 ? n : 1) + 15) / 16;
  uint64_t key;
  if (ntn <= max_ntn)
    key = (uint64_t)(ntn - 1) << kb.row_bits;
  else
    key = (1ull << (kb.row_bits + kb.n_bits)) | ((uint64_t)(max_n - n) << kb.row_bits);
  keys[r] = key | (uint64_t)r;
}

__global__ __launch_bounds__(FI_THREADS) void fold_expand_kernel(const uint64_t* keys,
                                                                 const int64_t* rowptr,
                                                                 int64_t nrows, FoldKeyBits kb,
                                                                 int64_t* order, RowDesc* desc,
                                                                 int64_t* wb) {
  const int64_t i = (int64_t)blockIdx.x * FI_THREADS + threadIdx.x;
  if (i >= nrows) return;
  const uint64_t key = keys[i];
  const int64_t row = (int64_t)(key & ((1ull << kb.row_bits) - 1));
  const int64_t beg = rowptr[row];
  order[i] = row;
  desc[i] = RowDesc{beg, (int32_t)(rowptr[row + 1] - beg), (int32_t)row};
  // the first slot of every class entered here (classes without rows included)
  const int cls = fold_class(key, kb);
  const int prev = i == 0 ? -1 : fold_class(keys[i - 1], kb);
  for (int b = prev + 1; b <= cls; ++b) wb[b] = i;
  if (i == nrows - 1)
    for (int b = cls + 1; b <= kMaxNTN; ++b) wb[b] = nrows;
}

template <typename T>
__global__ __launch_bounds__(FI_THREADS) void fold_gather_kernel(const T* X, int64_t nrows, int k,
                                                                 int kp, double* out) {
  const int64_t idx = (int64_t)blockIdx.x * FI_THREADS + threadIdx.x;
  if (idx >= nrows * k) return;
  const int64_t r = idx / k;
  const int f = (int)(idx - r * k);
  out[idx] = (double)X[r * kp + f];
}

__global__ __launch_bounds__(FI_THREADS) void iota_kernel(int64_t* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * FI_THREADS + threadIdx.x;
  if (i < n) out[i] = i;
}

template <typename T>
hipError_t gather(const T* X, int64_t nrows, int k, int kp, double* out, hipStream_t s) {
  if (nrows > 0)
    hipLaunchKernelGGL(fold_gather_kernel<T>, dim3(fi_blocks(nrows * k)), dim3(FI_THREADS), 0, s,
                       X, nrows, k, kp, out);
  return hipGetLastError();
}

}  // namespace

FoldKeyBits fold_key_bits(int64_t nrows, int64_t max_n) {
  const int rb = bit_width((uint64_t)(nrows > 1 ? nrows - 1 : 1));
  // the field holds max_n − n ≤ max_n and NTN − 1 < kMaxNTN
  const int nb = bit_width((uint64_t)(max_n > kMaxNTN - 1 ? max_n : kMaxNTN - 1));
  return FoldKeyBits{rb, nb};
}

hipError_t launch_fold_keys(const int64_t* rowptr, int64_t nrows, int max_ntn, int64_t max_n,
                            FoldKeyBits kb, uint64_t* keys, hipStream_t s) {
  if (kb.end_bit() > 64 || nrows > 0x7fffffffll) return hipErrorInvalidValue;
  if (nrows > 0)
    hipLaunchKernelGGL(fold_keys_kernel, dim3(fi_blocks(nrows)), dim3(FI_THREADS), 0, s, rowptr,
                       nrows, max_ntn, max_n, kb, keys);
  return hipGetLastError();
}

hipError_t launch_fold_expand(const uint64_t* keys, const int64_t* rowptr, int64_t nrows,
                              FoldKeyBits kb, int64_t* order, RowDesc* desc, int64_t* wb,
                              hipStream_t s) {
  if (nrows > 0)
    hipLaunchKernelGGL(fold_expand_kernel, dim3(fi_blocks(nrows)), dim3(FI_THREADS), 0, s, keys,
                       rowptr, nrows, kb, order, desc, wb);
  return hipGetLastError();
}

hipError_t launch_fold_gather(const float* X, int64_t nrows, int k, int kp, double* out,
                              hipStream_t s) {
  return gather(X, nrows, k, kp, out, s);
}
hipError_t launch_fold_gather(const double* X, int64_t nrows, int k, int kp, double* out,
                              hipStream_t s) {
  return gather(X, nrows, k, kp, out, s);
}

hipError_t launch_iota(int64_t* out, int64_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(iota_kernel, dim3(fi_blocks(n)), dim3(FI_THREADS), 0, s, out, n);
  return hipGetLastError();
}

}  // namespace qmfx
