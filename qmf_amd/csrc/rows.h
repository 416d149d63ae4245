// Rows solved against a fixed side: the one launch sequence behind a half's pieces
// (api_wals.cpp; the heavy rows of a CG half, api_wals_cg.cpp) and a fold-in (api_foldin.cpp), what precedes and follows it, and the rows a
// call brings as a CSR of their own (fold-in, qmfx_wals_explain_rows).
#pragma once
#include "ctx.h"

namespace qmfx {

// The fixed side's part of a half, from its current factors: G = YᵀY, and for the whitened
// rows (use_w) L⁻¹ of G + λI and Z = Y·L⁻ᵀ; G + λI's tile image for the one-wave direct rows.
template <typename T>
int fixed_side_prologue(qmfx_ctx* c, const SideBuf& R, double lambda, bool use_w) {
  // G = YᵀY of the fixed side (full replica on every rank)
  HIPCHK(launch_gram_t<T>(c, R));
  if (use_w) {
    if (c->z_cap < R.n) {
      // one extra all-zero row (index z_cap): the whitened kernel's padding signals
      const int64_t cap = std::max(c->s[0].n, c->s[1].n);
      HIPCHK(dev_alloc(c->Z, (size_t)(cap + 1) * c->kp * c->esz));
      HIPCHK(hipMemsetAsync(c->Z.as<char>() + (size_t)cap * c->kp * c->esz, 0,
                            (size_t)c->kp * c->esz, c->stream));
      c->z_cap = cap;
    }
    HIPCHK(hipMemsetAsync(c->chol_status, 0, 4, c->stream));
    HIPCHK(launch_chol_inv(c->G.as<const T>(), c->nt, c->k, lambda, c->Linv.as<T>(),
                           c->chol_status, c->chol_scratch, c->stream));
    HIPCHK(launch_whiten(R.F.as<const T>(), c->Z.as<T>(), nullptr, R.n, c->nt,
                         c->Linv.as<const T>(), nullptr, 0.0, false, c->cus, c->stream));
  }
  if (!use_big_rows(c))
    HIPCHK(launch_gimg(c->G.as<const T>(), c->nt, c->k, lambda, c->Gimg.as<T>(), c->stream));
  return 0;
}

// the per-row losses and status words of a half over n rows
inline int ensure_rowloss(qmfx_ctx* c, int64_t n) {
  if (c->rowloss_cap >= n) return 0;
  c->status.reset();
  HIPCHK(dev_alloc(c->rowloss, (size_t)std::max<int64_t>(n, 1) * sizeof(double)));
  HIPCHK(dev_alloc(c->status, (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t)));
  c->rowloss_cap = n;
  return 0;
}

// The rows being solved: their CSR, where their factors, losses and status words go, and
// their plan (order and desc are indexed by slot).
template <typename T>
struct Rows {
  const int64_t* rowptr;
  const int32_t* col;
  const T* val;
  T* X;
  double* rowloss;
  int32_t* status;
  const int64_t* order;
  const RowDesc* desc;
};
// a side of the context, solved by a half
template <typename T>
Rows<T> side_rows(qmfx_ctx* c, const SideBuf& L) {
  return {L.rowptr, colp(L), valp<T>(L), L.F.as<T>(), c->rowloss, c->status, L.d_order, L.d_desc};
}

// The split-K heavy rows among a launch sequence's direct slots (Piece): heavy indices and
// segments of side's d_seg / d_heavy / d_hseg lists.  No side: the rows have none (fold-in).
struct SplitK {
  const SideBuf* side = nullptr;
  int64_t nh = 0, h0 = 0, s0 = 0, ns = 0;
};

template <typename T>
FallbackArgs<T> fallback_args(qmfx_ctx* c, const Rows<T>& v, const SideBuf& R, int64_t slot_begin,
                              int64_t nslots, double alpha, double lambda) {
  FallbackArgs<T> a{};
  a.rowptr = v.rowptr;
  a.col = v.col;
  a.val = v.val;
  a.Y = R.F.as<T>();
  a.G = c->G.as<T>();
  a.X = v.X;
  a.rowloss = v.rowloss;
  a.status = v.status;
  a.desc = v.desc;
  a.slot_begin = slot_begin;
  a.nslots = nslots;
  a.alpha = alpha;
  a.lambda = lambda;
  a.k = c->k;
  a.kp = c->kp;
  a.scratch = c->fb_scratch;
  a.counters = c->fb_cnt;
  return a;
}

// The row kernels' arguments for `n` slots from `b` of the rows' order, gathering rows of Y.
template <typename T>
SolveArgs<T> solve_args(qmfx_ctx* c, const Rows<T>& v, const T* Y, int32_t zrow, int64_t b,
                        int64_t n, double alpha, double lambda, uint64_t* trace) {
  return SolveArgs<T>{v.rowptr, v.col, v.val, Y, nullptr, v.X, v.rowloss, v.status, v.order, b, n,
                      (T)alpha, (T)lambda, c->k, v.desc, nullptr, trace, zrow};
}

// The row solves of slots slot0 .. slot0 + nslots against R after fixed_side_prologue, in
// stream order: the direct rows (heaviest first; the split-K heavy rows lead; all rows when
// the whitened form is off), the whitened buckets (wb: their boundaries relative to slot0,
// wb[kMaxNTN] = the first direct slot) with x = L⁻ᵀx', then the pivoted re-solve of flagged
// rows.  `mid`, when given, is recorded between the direct and the whitened launches.
template <typename T>
int solve_rows(qmfx_ctx* c, const Rows<T>& v, const SideBuf& R, int64_t slot0, int64_t nslots,
               const int64_t* wb, double alpha, double lambda, bool use_w, const SplitK& sk = {},
               uint64_t* trace = nullptr, hipEvent_t mid = nullptr) {
  // one launch of the direct-row kernels: seg_mode 0 = slots of the order (rows), 1 = split-K
  // segments (d_seg), 2 = split-K heavy-row solves (d_heavy)
  auto direct = [&](int64_t b, int64_t n, int mode) {
    if (n <= 0) return 0;
    SolveArgs<T> a = solve_args<T>(c, v, R.F.as<T>(), (int32_t)R.n, b, n, alpha, lambda,
                                   mode == 0 ? trace : nullptr);
    a.G = c->G.as<T>();
    a.Gimg = c->Gimg.as<T>();
    a.seg_mode = mode;
    if (sk.side) {
      a.desc = mode == 1 ? sk.side->d_seg.get() : mode == 2 ? sk.side->d_heavy.get() : v.desc;
      a.part = c->part.as<T>();
      a.partb = c->partb.as<T>();
      a.partc = c->partc;
    }
    const hipError_t e = use_big_rows(c) ? launch_wals_big(a, c->nt, c->stream)
                                         : launch_wals_direct(a, c->nt, c->stream);
    if (e != hipSuccess) return fail(std::string("row kernel launch: ") + hipGetErrorString(e), -2);
    return 0;
  };
  const int64_t nW = wb[kMaxNTN], dh = slot0 + nW;
  if (sk.nh > 0) {
    // heavy rows: segment Grams (one wave per segment), fixed-order fp64 reduction into
    // each row's first segment, then the row solves from those images
    if (int rc = direct(sk.s0, sk.ns, 1)) return rc;
    if (use_big_rows(c))
      // multi-wave tilings: G + λI's image is built here (the direct kernels' Gimg is not)
      HIPCHK(launch_heavy_reduce_big(c->part.as<T>(), c->partb.as<T>(), c->partc, sk.side->d_hseg,
                                     sk.h0, sk.nh, c->G.as<const T>(), c->Gimg.as<T>(), c->nt,
                                     c->k, lambda, c->stream));
    else
      HIPCHK(launch_heavy_reduce(c->part.as<T>(), c->partb.as<T>(), c->partc, sk.side->d_hseg,
                                 sk.h0, sk.nh, c->Gimg.as<const T>(), c->nt, c->stream));
    if (int rc = direct(sk.h0, sk.nh, 2)) return rc;
  }
  if (!use_w)
    if (int rc = direct(slot0, nW, 0)) return rc;
  if (int rc = direct(dh + sk.nh, slot0 + nslots - dh - sk.nh, 0)) return rc;
  if (mid) HIPCHK(hipEventRecord(mid, c->stream));
  // whitened rows: per-bucket row solve, then x = L⁻ᵀ x' and −λ‖x‖²
  if (use_w && nW > 0) {
    for (int b = 0; b < kMaxNTN; ++b) {
      const int64_t cnt = wb[b + 1] - wb[b];
      if (cnt <= 0) continue;
      HIPCHK(launch_wals_woodbury(solve_args<T>(c, v, c->Z.as<T>(), (int32_t)c->z_cap,
                                                slot0 + wb[b], cnt, alpha, lambda, trace),
                                  c->nt, b + 1, c->stream));
    }
    HIPCHK(launch_whiten(v.X, v.X, v.order + slot0, nW, c->nt, c->Linv.as<const T>(), v.rowloss,
                         lambda, true, c->cus, c->stream));
  }
  // rows the Cholesky kernels flagged: pivoted fp64 re-solve
  if (nslots > 0)
    HIPCHK(launch_wals_fallback(fallback_args<T>(c, v, R, slot0, nslots, alpha, lambda), c->stream));
  return 0;
}

// After the last launch: the end-of-half status block in hsum ([0] loss, [1] rows re-solved,
// [2] singular rows, [3] factorization flag; one small copy into pinned memory).  The stream
// is idle when this returns.
inline int read_half_status(qmfx_ctx* c) {
  HIPCHK(hipMemcpyAsync(c->hsum, c->dsum + kHalfStatus, 4 * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
// the failures it reports; the first is the reference's CHECK(info == 0) after dsysv_
// (Matrix.cpp:94)
inline int half_status_failure(const qmfx_ctx* c) {
  if (c->hsum[2] != 0.0)
    return fail(std::to_string((int64_t)c->hsum[2]) + " singular row system(s) (dsysv info > 0)", -6);
  if (c->hsum[3] != 0.0) return fail("YᵀY + λI is not positive definite", -5);
  return 0;
}

// algorithmic work of nr rows with nz signals on the direct kernels: the k×k form of every row
inline double direct_flops(const qmfx_ctx* c, double nz, double nr) {
  const double k = c->k;
  return nz * k * (k + 1) + nz * 2 * k + nr * (k * k * k / 3.0 + 2 * k * k);
}
inline double direct_bytes(const qmfx_ctx* c, double nz, double nr) {
  const double k = c->k, s = (double)c->esz;
  return nz * (4 + s) + nz * k * s + nr * k * s + (nr + 1) * 8;
}

// The one host pass over rows given as a CSR of their own: the CSR's shape and every column
// index (an index out of range would be a device fault).  *max_n: the longest row.
// need_values = false: the rows carry no values (qmfx_bpr_fold_in's positives).
inline int validate_rows(int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
                         const double* values, int64_t nother, bool need_ascending,
                         int64_t* max_n, bool need_values = true) {
  if (nrows < 0 || nrows > 0x7fffffffll) return fail("nrows out of range (at most 2^31-1 rows)");
  if (!rowptr) return fail("rowptr is null");
  if (rowptr[0] != 0) return fail("rowptr[0] must be 0");
  int64_t mx = 0;
  for (int64_t r = 0; r < nrows; ++r) {
    if (rowptr[r + 1] < rowptr[r]) return fail("rowptr not monotone");
    mx = std::max(mx, rowptr[r + 1] - rowptr[r]);
  }
  const int64_t nnz = rowptr[nrows];
  if (nnz > 0x7fffffffll) return fail("at most 2^31-1 signals in one fold-in call");
  if (nnz > 0 && (!colidx || (need_values && !values))) return fail("colidx or values is null");
  for (int64_t e = 0; e < nnz; ++e)
    if (colidx[e] < 0 || colidx[e] >= nother) return fail("column index out of range");
  if (need_ascending)
    for (int64_t r = 0; r < nrows; ++r)
      for (int64_t e = rowptr[r] + 1; e < rowptr[r + 1]; ++e)
        if (colidx[e] < colidx[e - 1])
          return fail("exclude_seen needs the column indices ascending within a row");
  *max_n = mx;
  return 0;
}
// validated rows → fr_rowptr / fr_col / fr_val (values in the context precision; none when
// `values` is null)
inline int upload_rows(qmfx_ctx* c, int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
                       const double* values) {
  const size_t n1 = (size_t)nrows, nnz = (size_t)rowptr[nrows], m1 = std::max<size_t>(nnz, 1);
  if (int rc = reserve(c->fr_rowptr, (n1 + 1) * 8)) return rc;
  if (int rc = reserve(c->fr_col, m1 * 4)) return rc;
  if (values || nnz == 0)
    if (int rc = reserve(c->fr_val, m1 * c->esz)) return rc;
  HIPCHK(scopy(c, c->fr_rowptr, rowptr, (n1 + 1) * 8, hipMemcpyHostToDevice));
  if (nnz > 0) {
    HIPCHK(scopy(c, c->fr_col, colidx, nnz * 4, hipMemcpyHostToDevice));
    if (values) HIPCHK(copy_in(c, c->fr_val, values, nnz));
  }
  return 0;
}

}  // namespace qmfx
