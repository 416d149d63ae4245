// BPR fold-in: new users' rows fitted by SGD against the context's frozen item factors and
// biases (bpr_foldin.hip), and their top-N recommendations.  The rows arrive as a CSR of their
// own through the fold-in upload and scratch (rows.h, ctx.h fr_* / fi_*).
#include "rows.h"

using namespace qmfx;

namespace {

struct Schedule {
  uint64_t seed;
  int nepochs, num_neg;
  double lr, decay, user_lambda;
  int use_biases;
};

// everything the calls reject, before the device is touched
int bpr_fold_checks(qmfx_ctx* c, int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
                    const Schedule& s) {
  if (!c) return fail("null context");
  if (!c->s[1].F) return fail("no item factors (qmfx_set_shape and qmfx_set_factors first)");
  if (s.use_biases && !c->bias) return fail("no item biases on the context");
  if (c->k > 256) return fail("BPR fold-in supports nfactors <= 256");
  if (s.nepochs < 1) return fail("nepochs must be at least 1");
  if (s.num_neg < 1) return fail("num_neg must be at least 1");
  int64_t max_n = 0;
  if (int rc = validate_rows(nrows, rowptr, colidx, nullptr, c->s[1].n, false, &max_n, false))
    return rc;
  // the rejection test of a draw and exclude_seen both take a row as a sorted set
  for (int64_t r = 0; r < nrows; ++r)
    for (int64_t e = rowptr[r] + 1; e < rowptr[r + 1]; ++e)
      if (colidx[e] <= colidx[e - 1])
        return fail("the item indices of a row must be strictly ascending");
  return 0;
}

// Uploads the rows and their start values and enqueues the kernel (validated input, nrows > 0).
// Records ev0 in front of the kernel; leaves the rows in fi_X (padded, context precision) and
// their losses in fi_rowloss.
template <typename T>
int bpr_fold_t(qmfx_ctx* c, int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
               const double* init, const Schedule& s) {
  const size_t n1 = (size_t)nrows, kp = (size_t)c->kp, k = (size_t)c->k;
  if (int rc = upload_rows(c, nrows, rowptr, colidx, nullptr)) return rc;
  if (int rc = reserve(c->fi_X, n1 * kp * c->esz)) return rc;
  if (int rc = reserve(c->fi_rowloss, n1 * 8)) return rc;
  if (int rc = reserve(c->fi_lr, (size_t)s.nepochs * c->esz)) return rc;
  // BPREngine::optimize's rule in double, every pass's rate rounded once
  std::vector<T> lrs((size_t)s.nepochs);
  double lr = s.lr;
  for (int e = 0; e < s.nepochs; ++e, lr *= s.decay) lrs[e] = (T)lr;
  HIPCHK(scopy(c, c->fi_lr, lrs.data(), lrs.size() * sizeof(T), hipMemcpyHostToDevice));
  if (init) {
    std::vector<T> x(n1 * kp, T(0));  // the padding columns stay 0
    for (size_t r = 0; r < n1; ++r)
      for (size_t f = 0; f < k; ++f) x[r * kp + f] = (T)init[r * k + f];
    HIPCHK(scopy(c, c->fi_X, x.data(), x.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemsetAsync(c->bad, 0, 4, c->stream));
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  if (!init) HIPCHK(hipMemsetAsync(c->fi_X, 0, n1 * kp * c->esz, c->stream));
  BprFoldArgs<T> a{};
  a.I = c->s[1].F.as<T>();
  a.bias = s.use_biases ? c->bias.as<T>() : nullptr;
  a.rowptr = c->fr_rowptr;
  a.col = c->fr_col;
  a.X = c->fi_X.as<T>();
  a.losses = c->fi_rowloss;
  a.lr = c->fi_lr.as<T>();
  a.nrows = nrows;
  a.nitems = c->s[1].n;
  a.nepochs = s.nepochs;
  a.num_neg = s.num_neg;
  a.seed = s.seed;
  a.user_lambda = (T)s.user_lambda;
  a.kp = c->kp;
  a.bad = c->bad;
  a.grid = bpr_fold_grid(nrows);
  HIPCHK(launch_bpr_fold(a, c->stream));
  return 0;
}

// after ev1: the non-finite flag and the call's kernel time with its work, steps × 6k flop and
// steps × two item rows
int bpr_fold_finish(qmfx_ctx* c, int64_t nnz, const Schedule& s, double extra_flops,
                    double extra_bytes, int32_t* bad) {
  HIPCHK(hipMemcpyAsync(bad, c->bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  const double steps = (double)s.nepochs * (double)s.num_neg * (double)nnz;
  c->solve.add(ms, steps * 6.0 * c->k + extra_flops,
               steps * 2.0 * c->kp * (double)c->esz + extra_bytes);
  return 0;
}

}  // namespace

extern "C" {

int qmfx_bpr_fold_in(qmfx_ctx* c, int64_t nrows, const int64_t* rowptr, const int32_t* colidx,
                     const double* init, uint64_t seed, int nepochs, int num_neg, double lr,
                     double decay, double user_lambda, int use_biases, double* factors,
                     double* losses) {
  const Schedule s{seed, nepochs, num_neg, lr, decay, user_lambda, use_biases};
  if (int rc = bpr_fold_checks(c, nrows, rowptr, colidx, s)) return rc;
  if (nrows == 0) return 0;
  if (!factors) return fail("factors is null");
  if (set_dev(c)) return -2;
  const size_t out = (size_t)nrows * (size_t)c->k;
  if (int rc = reserve(c->fi_out, out * 8)) return rc;
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    if (int r = bpr_fold_t<T>(c, nrows, rowptr, colidx, init, s)) return r;
    HIPCHK(launch_fold_gather(c->fi_X.as<const T>(), nrows, c->k, c->kp, c->fi_out, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  int32_t bad = 0;
  if (int r = bpr_fold_finish(c, rowptr[nrows], s, 0.0, 0.0, &bad)) return r;
  HIPCHK(scopy(c, factors, c->fi_out, out * 8, hipMemcpyDeviceToHost));
  if (losses) HIPCHK(scopy(c, losses, c->fi_rowloss, (size_t)nrows * 8, hipMemcpyDeviceToHost));
  if (bad) return fail(kBadGradients, -4);
  return 0;
}

int qmfx_bpr_recommend_fold_in(qmfx_ctx* c, int64_t nrows, const int64_t* rowptr,
                               const int32_t* colidx, const double* init, uint64_t seed,
                               int nepochs, int num_neg, double lr, double decay,
                               double user_lambda, int use_biases, int topn, int exclude_seen,
                               int64_t* items, double* scores, int32_t* counts, double* factors) {
  const Schedule s{seed, nepochs, num_neg, lr, decay, user_lambda, use_biases};
  if (topn < 1 || topn > QMFX_REC_MAX_N) return fail("topn must be in 1..128 (QMFX_REC_MAX_N)");
  if (int rc = bpr_fold_checks(c, nrows, rowptr, colidx, s)) return rc;
  if (nrows == 0) return 0;
  if (!items || !scores || !counts) return fail("items, scores or counts is null");
  if (set_dev(c)) return -2;
  const int64_t ni = c->s[1].n;
  const size_t fout = (size_t)nrows * (size_t)c->k;
  if (factors)
    if (int rc = reserve(c->fi_out, fout * 8)) return rc;
  if (int rc = topn_reserve(c, nrows, ni, topn)) return rc;
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    if (int r = bpr_fold_t<T>(c, nrows, rowptr, colidx, init, s)) return r;
    if (factors)
      HIPCHK(launch_fold_gather(c->fi_X.as<const T>(), nrows, c->k, c->kp, c->fi_out, c->stream));
    HIPCHK(launch_iota(c->rc.users, nrows, c->stream));
    // qmfx_recommend's selection with the folded rows as the users and their positives as seen
    RecArgs<T> a{};
    topn_args(c, a, nrows, ni, topn);
    a.U = c->fi_X.as<T>();
    a.I = c->s[1].F.as<T>();
    a.bias = use_biases ? c->bias.as<T>() : nullptr;
    if (exclude_seen) {
      a.seen_ptr = c->fr_rowptr;
      a.seen_col = c->fr_col;
    }
    HIPCHK(launch_recommend(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  int32_t bad = 0;
  if (int r = bpr_fold_finish(c, rowptr[nrows], s, topn_flops(c, nrows, ni),
                              topn_bytes(c, nrows, ni), &bad))
    return r;
  if (int r = topn_copy_out(c, nrows, topn, items, scores, counts)) return r;
  if (factors) HIPCHK(scopy(c, factors, c->fi_out, fout * 8, hipMemcpyDeviceToHost));
  if (bad) return fail(kBadGradients, -4);
  return 0;
}

}  // extern "C"
