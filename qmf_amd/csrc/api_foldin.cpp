// Fold-in: rows that were not in the training matrix, solved from their signals against the
// context's current factors of the other side, and their top-N recommendations.  The rows go
// through a half's launch sequence (solve_rows, rows.h) as a view of the uploaded CSR and the
// fold-in scratch; their plan is built on the device (foldin.hip).
#include "rows.h"

using namespace qmfx;

namespace {

// Uploads the rows, plans them and enqueues their solves (validated input, nrows > 0).
// Records ev0 in front of the first kernel; leaves the rows in fi_X (padded, context
// precision), their losses in fi_rowloss and the end-of-half status block in dsum.
template <typename T>
int fold_in_t(qmfx_ctx* c, int side, int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
              const double* values, int64_t max_n, double alpha, double lambda) {
  const SideBuf& R = c->s[1 - side];
  const size_t n1 = (size_t)nrows;
  c->fi_n = -1;
  if (int rc = upload_rows(c, nrows, rowptr, colidx, values)) return rc;
  if (int rc = reserve(c->fi_X, n1 * c->kp * c->esz)) return rc;
  if (int rc = reserve(c->fi_rowloss, n1 * 8)) return rc;
  if (int rc = reserve(c->fi_status, n1 * 4)) return rc;
  if (int rc = reserve(c->fi_keys, n1 * 8)) return rc;
  if (int rc = reserve(c->fi_keys2, n1 * 8)) return rc;
  if (int rc = reserve(c->fi_order, n1 * 8)) return rc;
  if (int rc = reserve(c->fi_desc, n1 * sizeof(RowDesc))) return rc;
  if (int rc = reserve(c->fi_wb, (kMaxNTN + 1) * 8)) return rc;
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  // the rows start from 0, as a side's factors do (the padding columns stay 0)
  HIPCHK(hipMemsetAsync(c->fi_X, 0, n1 * c->kp * c->esz, c->stream));

  // the plan: keys, one sort, order + descriptors + bucket boundaries
  const int mx = max_whitened_ntn(c);
  const FoldKeyBits kb = fold_key_bits(nrows, max_n);
  HIPCHK(launch_fold_keys(c->fr_rowptr, nrows, mx, max_n, kb, c->fi_keys, c->stream));
  HIPCHK(sort_keys(c->fi_keys, c->fi_keys2, nrows, kb.end_bit(), c->stream));
  HIPCHK(launch_fold_expand(c->fi_keys, c->fr_rowptr, nrows, kb, c->fi_order, c->fi_desc, c->fi_wb,
                            c->stream));
  int64_t wb[kMaxNTN + 1];
  HIPCHK(scopy(c, wb, c->fi_wb, sizeof(wb), hipMemcpyDeviceToHost));
  for (int b = 0; b < kMaxNTN; ++b) c->fi_classes[b] = wb[b + 1] - wb[b];
  c->fi_classes[kMaxNTN] = nrows - wb[kMaxNTN];
  c->fi_classes[kMaxNTN + 1] = c->fi_classes[kMaxNTN + 2] = 0;
  c->fi_n = nrows;

  const bool use_w = wb[kMaxNTN] > 0 && lambda > 0.0;
  if (int rc = fixed_side_prologue<T>(c, R, lambda, use_w)) return rc;
  HIPCHK(hipMemsetAsync(c->fi_status, 0, n1 * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->fb_cnt, 0, 2 * sizeof(unsigned long long), c->stream));
  // a half's row solves, of one piece of any row length without split-K rows
  const Rows<T> rows{c->fr_rowptr, c->fr_col, c->fr_val.as<T>(), c->fi_X.as<T>(), c->fi_rowloss,
                     c->fi_status, c->fi_order, c->fi_desc};
  if (int rc = solve_rows<T>(c, rows, R, 0, nrows, wb, alpha, lambda, use_w)) return rc;
  // re-solve counts and the factorization flag in the half's status block ([0] unused here)
  HIPCHK(launch_half_status(c->dsum, c->fb_cnt, use_w ? c->chol_status.get() : nullptr,
                            c->dsum + kHalfStatus, c->stream));
  return 0;
}

int fold_in_checks(qmfx_ctx* c, int side) {
  if (!c) return fail("null context");
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  if (!c->s[1 - side].F) return fail("no factors on the fixed side (qmfx_set_shape and qmfx_set_factors first)");
  return 0;
}

// after ev1: the status block, the call's kernel time, the failures of a half
int fold_in_finish(qmfx_ctx* c, int64_t nrows, int64_t nnz, double extra_flops, double extra_bytes,
                   int64_t* pivoted) {
  if (int rc = read_half_status(c)) return rc;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  // every row counted on the direct kernels, as half_end counts its direct class
  c->solve.add(ms, direct_flops(c, (double)nnz, (double)nrows) + extra_flops,
               direct_bytes(c, (double)nnz, (double)nrows) + extra_bytes);
  if (pivoted) *pivoted = (int64_t)c->hsum[1];
  return half_status_failure(c);
}

}  // namespace

extern "C" {

int qmfx_wals_fold_in(qmfx_ctx* c, int side, int64_t nrows, const int64_t* rowptr,
                      const int32_t* colidx, const double* values, double alpha, double lambda,
                      double* factors, double* losses, int64_t* pivoted) {
  if (int rc = fold_in_checks(c, side)) return rc;
  int64_t max_n = 0;
  if (int rc = validate_rows(nrows, rowptr, colidx, values, c->s[1 - side].n, false, &max_n)) return rc;
  if (pivoted) *pivoted = 0;
  if (nrows == 0) return 0;
  if (!factors) return fail("factors is null");
  if (set_dev(c)) return -2;
  const size_t out = (size_t)nrows * (size_t)c->k;
  if (int rc = reserve(c->fi_out, out * 8)) return rc;
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    if (int r = fold_in_t<T>(c, side, nrows, rowptr, colidx, values, max_n, alpha, lambda)) return r;
    HIPCHK(launch_fold_gather(c->fi_X.as<const T>(), nrows, c->k, c->kp, c->fi_out, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  if (int r = fold_in_finish(c, nrows, rowptr[nrows], 0.0, 0.0, pivoted)) return r;
  HIPCHK(scopy(c, factors, c->fi_out, out * 8, hipMemcpyDeviceToHost));
  if (losses) HIPCHK(scopy(c, losses, c->fi_rowloss, (size_t)nrows * 8, hipMemcpyDeviceToHost));
  return 0;
}

int qmfx_fold_in_classes(qmfx_ctx* c, int64_t* counts) {
  if (!c || c->fi_n < 0) return fail("no fold-in planned yet");
  std::copy(c->fi_classes, c->fi_classes + kMaxNTN + 3, counts);
  return 0;
}

int qmfx_fold_in_order(qmfx_ctx* c, int64_t* order) {
  if (!c || c->fi_n < 0) return fail("no fold-in planned yet");
  if (set_dev(c)) return -2;
  HIPCHK(scopy(c, order, c->fi_order, (size_t)c->fi_n * 8, hipMemcpyDeviceToHost));
  return 0;
}

int qmfx_recommend_fold_in(qmfx_ctx* c, int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
                           const double* values, double alpha, double lambda, int topn,
                           int exclude_seen, int64_t* items, double* scores, int32_t* counts,
                           double* factors) {
  if (int rc = fold_in_checks(c, 0)) return rc;
  if (topn < 1 || topn > QMFX_REC_MAX_N) return fail("topn must be in 1..128 (QMFX_REC_MAX_N)");
  int64_t max_n = 0;
  const int64_t ni = c->s[1].n;
  if (int rc = validate_rows(nrows, rowptr, colidx, values, ni, exclude_seen != 0, &max_n)) return rc;
  if (nrows == 0) return 0;
  if (!items || !scores || !counts) return fail("items, scores or counts is null");
  if (set_dev(c)) return -2;
  const size_t fout = (size_t)nrows * (size_t)c->k;
  if (factors)
    if (int rc = reserve(c->fi_out, fout * 8)) return rc;
  if (int rc = topn_reserve(c, nrows, ni, topn)) return rc;
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    if (int r = fold_in_t<T>(c, 0, nrows, rowptr, colidx, values, max_n, alpha, lambda)) return r;
    if (factors)
      HIPCHK(launch_fold_gather(c->fi_X.as<const T>(), nrows, c->k, c->kp, c->fi_out, c->stream));
    HIPCHK(launch_iota(c->rc.users, nrows, c->stream));
    // qmfx_recommend's selection with the folded rows as the users and their signals as seen
    RecArgs<T> a{};
    topn_args(c, a, nrows, ni, topn);
    a.U = c->fi_X.as<T>();
    a.I = c->s[1].F.as<T>();
    if (exclude_seen) {
      a.seen_ptr = c->fr_rowptr;
      a.seen_col = c->fr_col;
    }
    HIPCHK(launch_recommend(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  if (int r = fold_in_finish(c, nrows, rowptr[nrows], topn_flops(c, nrows, ni),
                             topn_bytes(c, nrows, ni), nullptr))
    return r;
  if (int r = topn_copy_out(c, nrows, topn, items, scores, counts)) return r;
  if (factors) HIPCHK(scopy(c, factors, c->fi_out, fout * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
