// Fold-in: rows that were not in the training matrix, solved from their signals against the
// context's current factors of the other side, and their top-N recommendations.  The rows go
// through the row kernels of a half (api_wals.cpp) with the arguments pointing at the uploaded
// CSR and the fold-in scratch; their plan is built on the device (foldin.hip).
#include "ctx.h"

using namespace qmfx;

// The one host pass over the new rows (ctx.h; qmfx_wals_explain_rows validates with it too).
int qmfx::validate_rows(int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
                        const double* values, int64_t nother, bool need_ascending,
                        int64_t* max_n) {
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
  if (nnz > 0 && (!colidx || !values)) return fail("colidx or values is null");
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

namespace {

// Uploads the rows, plans them and enqueues their solves (validated input, nrows > 0).
// Records ev0 in front of the first kernel; leaves the rows in fi_X (padded, context
// precision), their losses in fi_rowloss and the end-of-half status block in dsum.
template <typename T>
int fold_in_t(qmfx_ctx* c, int side, int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
              const double* values, int64_t max_n, double alpha, double lambda) {
  const SideBuf& R = c->s[1 - side];
  const int64_t nnz = rowptr[nrows];
  const size_t n1 = (size_t)nrows, m1 = (size_t)std::max<int64_t>(nnz, 1);
  if (int rc = grow(c->fi_rowptr, c->fi_cap[0], (n1 + 1) * 8)) return rc;
  if (int rc = grow(c->fi_col, c->fi_cap[1], m1 * 4)) return rc;
  if (int rc = grow(c->fi_val, c->fi_cap[2], m1 * c->esz)) return rc;
  if (int rc = grow(c->fi_X, c->fi_cap[3], n1 * c->kp * c->esz)) return rc;
  if (int rc = grow(c->fi_rowloss, c->fi_cap[4], n1 * 8)) return rc;
  if (int rc = grow(c->fi_status, c->fi_cap[5], n1 * 4)) return rc;
  if (int rc = grow(c->fi_keys, c->fi_cap[6], n1 * 8)) return rc;
  if (int rc = grow(c->fi_keys2, c->fi_cap[7], n1 * 8)) return rc;
  if (int rc = grow(c->fi_order, c->fi_cap[8], n1 * 8)) return rc;
  if (int rc = grow(c->fi_desc, c->fi_cap[9], n1 * sizeof(RowDesc))) return rc;
  if (int rc = grow(c->fi_wb, c->fi_cap[10], (kMaxNTN + 1) * 8)) return rc;
  c->fi_n = -1;
  HIPCHK(scopy(c, c->fi_rowptr, rowptr, (n1 + 1) * 8, hipMemcpyHostToDevice));
  if (nnz > 0) {
    HIPCHK(scopy(c, c->fi_col, colidx, (size_t)nnz * 4, hipMemcpyHostToDevice));
    HIPCHK(copy_in(c, c->fi_val, values, (size_t)nnz));
  }
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  // the rows start from 0, as a side's factors do (the padding columns stay 0)
  HIPCHK(hipMemsetAsync(c->fi_X, 0, n1 * c->kp * c->esz, c->stream));

  // the plan: keys, one sort, order + descriptors + bucket boundaries
  const int mx = max_whitened_ntn(c);
  const FoldKeyBits kb = fold_key_bits(nrows, max_n);
  HIPCHK(launch_fold_keys(c->fi_rowptr, nrows, mx, max_n, kb, c->fi_keys, c->stream));
  HIPCHK(sort_keys(c->fi_keys, c->fi_keys2, nrows, kb.end_bit(), c->stream));
  HIPCHK(launch_fold_expand(c->fi_keys, c->fi_rowptr, nrows, kb, c->fi_order, c->fi_desc, c->fi_wb,
                            c->stream));
  int64_t wb[kMaxNTN + 1];
  HIPCHK(scopy(c, wb, c->fi_wb, sizeof(wb), hipMemcpyDeviceToHost));
  for (int b = 0; b < kMaxNTN; ++b) c->fi_classes[b] = wb[b + 1] - wb[b];
  c->fi_classes[kMaxNTN] = nrows - wb[kMaxNTN];
  c->fi_classes[kMaxNTN + 1] = c->fi_classes[kMaxNTN + 2] = 0;
  c->fi_n = nrows;

  const int64_t nW = wb[kMaxNTN];
  const bool use_w = nW > 0 && lambda > 0.0;
  if (int rc = fixed_side_prologue<T>(c, R, lambda, use_w)) return rc;
  HIPCHK(hipMemsetAsync(c->fi_status, 0, n1 * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->fb_cnt, 0, 2 * sizeof(unsigned long long), c->stream));

  auto args = [&](const T* Y, int32_t zrow, int64_t b, int64_t n) {
    return SolveArgs<T>{c->fi_rowptr, c->fi_col, c->fi_val.as<T>(), Y, nullptr, c->fi_X.as<T>(),
                        c->fi_rowloss, c->fi_status, c->fi_order, b, n, (T)alpha, (T)lambda, c->k,
                        c->fi_desc, nullptr, nullptr, zrow};
  };
  // direct rows, any length in one piece (seg_mode 0); all rows when the whitened form is off
  auto direct = [&](int64_t b, int64_t n) {
    if (n <= 0) return 0;
    SolveArgs<T> a = args(R.F.as<T>(), (int32_t)R.n, b, n);
    a.G = c->G.as<T>();
    a.Gimg = c->Gimg.as<T>();
    a.seg_mode = 0;
    const hipError_t e = use_big_rows(c) ? launch_wals_big(a, c->nt, c->stream)
                                         : launch_wals_direct(a, c->nt, c->stream);
    if (e != hipSuccess) return fail(std::string("row kernel launch: ") + hipGetErrorString(e), -2);
    return 0;
  };
  if (!use_w)
    if (int rc = direct(0, nW)) return rc;
  if (int rc = direct(nW, nrows - nW)) return rc;
  if (use_w) {
    for (int b = 0; b < kMaxNTN; ++b) {
      const int64_t cnt = wb[b + 1] - wb[b];
      if (cnt <= 0) continue;
      HIPCHK(launch_wals_woodbury(args(c->Z.as<T>(), (int32_t)c->z_cap, wb[b], cnt), c->nt, b + 1,
                                  c->stream));
    }
    HIPCHK(launch_whiten(c->fi_X.as<const T>(), c->fi_X.as<T>(), c->fi_order, nW, c->nt,
                         c->Linv.as<const T>(), c->fi_rowloss, lambda, true, c->cus, c->stream));
  }
  // rows the Cholesky kernels flagged: pivoted fp64 re-solve
  FallbackArgs<T> f{};
  f.rowptr = c->fi_rowptr;
  f.col = c->fi_col;
  f.val = c->fi_val.as<T>();
  f.Y = R.F.as<T>();
  f.G = c->G.as<T>();
  f.X = c->fi_X.as<T>();
  f.rowloss = c->fi_rowloss;
  f.status = c->fi_status;
  f.desc = c->fi_desc;
  f.slot_begin = 0;
  f.nslots = nrows;
  f.alpha = alpha;
  f.lambda = lambda;
  f.k = c->k;
  f.kp = c->kp;
  f.scratch = c->fb_scratch;
  f.counters = c->fb_cnt;
  HIPCHK(launch_wals_fallback(f, c->stream));
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
  HIPCHK(hipMemcpyAsync(c->hsum, c->dsum + kHalfStatus, 4 * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  // algorithmic work as the k×k form of every row (half_end's direct class)
  const double k = c->k, s = (double)c->esz, nz = (double)nnz, nr = (double)nrows;
  c->solve.add(ms, nz * k * (k + 1) + nz * 2 * k + nr * (k * k * k / 3.0 + 2 * k * k) + extra_flops,
               nz * (4 + s) + nz * k * s + nr * k * s + (nr + 1) * 8 + extra_bytes);
  if (pivoted) *pivoted = (int64_t)c->hsum[1];
  if (c->hsum[2] != 0.0)
    return fail(std::to_string((int64_t)c->hsum[2]) + " singular row system(s) (dsysv info > 0)", -6);
  if (c->hsum[3] != 0.0) return fail("YᵀY + λI is not positive definite", -5);
  return 0;
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
  if (int rc = grow(c->fi_out, c->fi_cap[11], out * 8)) return rc;
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
  const size_t lists = (size_t)(eval_chunks(nrows, ni) * eval_user_rows(nrows));
  const size_t out = (size_t)nrows * (size_t)topn, fout = (size_t)nrows * (size_t)c->k;
  if (factors)
    if (int rc = grow(c->fi_out, c->fi_cap[11], fout * 8)) return rc;
  if (int rc = grow(c->rc_users, c->rc_cap[0], (size_t)nrows * 8)) return rc;
  if (int rc = grow(c->rc_items, c->rc_cap[1], out * 8)) return rc;
  if (int rc = grow(c->rc_udbl, c->rc_cap[2], (size_t)(eval_user_rows(nrows) * c->k) * 8)) return rc;
  if (int rc = grow(c->rc_pscore, c->rc_cap[3], lists * (size_t)topn * 8)) return rc;
  if (int rc = grow(c->rc_scores, c->rc_cap[4], out * 8)) return rc;
  if (int rc = grow(c->rc_pitem, c->rc_cap[5], lists * (size_t)topn * 4)) return rc;
  if (int rc = grow(c->rc_pcnt, c->rc_cap[6], lists * 4)) return rc;
  if (int rc = grow(c->rc_counts, c->rc_cap[7], (size_t)nrows * 4)) return rc;
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    if (int r = fold_in_t<T>(c, 0, nrows, rowptr, colidx, values, max_n, alpha, lambda)) return r;
    if (factors)
      HIPCHK(launch_fold_gather(c->fi_X.as<const T>(), nrows, c->k, c->kp, c->fi_out, c->stream));
    HIPCHK(launch_iota(c->rc_users, nrows, c->stream));
    // qmfx_recommend's selection with the folded rows as the users and their signals as seen
    RecArgs<T> a{};
    a.U = c->fi_X.as<T>();
    a.I = c->s[1].F.as<T>();
    a.users = c->rc_users;
    a.nreq = nrows;
    a.nitems = ni;
    a.k = c->k;
    a.kp = c->kp;
    a.topn = topn;
    if (exclude_seen) {
      a.seen_ptr = c->fi_rowptr;
      a.seen_col = c->fi_col;
    }
    a.udbl = c->rc_udbl;
    a.part_score = c->rc_pscore;
    a.part_item = c->rc_pitem;
    a.part_cnt = c->rc_pcnt;
    a.items = c->rc_items;
    a.scores = c->rc_scores;
    a.counts = c->rc_counts;
    HIPCHK(launch_recommend(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  if (int r = fold_in_finish(c, nrows, rowptr[nrows], 2.0 * (double)nrows * (double)ni * c->k,
                             (double)((nrows + 31) / 32) * (double)ni * c->k * (double)c->esz,
                             nullptr))
    return r;
  HIPCHK(scopy(c, items, c->rc_items, out * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, scores, c->rc_scores, out * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, counts, c->rc_counts, (size_t)nrows * 4, hipMemcpyDeviceToHost));
  if (factors) HIPCHK(scopy(c, factors, c->fi_out, fout * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
