// Explanations: the per-signal contributions to y_tᵀA⁻¹b of a row's system, for rows of the
// context's own CSR (qmfx_wals_explain) or rows given as a CSR of their own
// (qmfx_wals_explain_rows).  One kernel (explain.hip) after the fixed side's YᵀY.
#include "rows.h"

using namespace qmfx;

namespace {

struct Outputs {
  int64_t *sources, *positions;
  double* contribs;
  int32_t* counts;
  double *totals, *all;
};

// what both forms check before anything is launched; *npairs = qptr[nq]
int explain_checks(qmfx_ctx* c, int side, int64_t nq, const int64_t* qptr, const int64_t* targets,
                   int topm, int64_t* npairs) {
  if (!c) return fail("null context");
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  if (topm < 1 || topm > QMFX_REC_MAX_N) return fail("topm must be in 1..128 (QMFX_REC_MAX_N)");
  if (!c->s[1 - side].F)
    return fail("no factors on the other side (qmfx_set_shape and qmfx_set_factors first)");
  if (c->k > 256) return fail("explanations support at most 256 factors");
  if (nq < 0 || nq > 0x7fffffffll) return fail("nq out of range (at most 2^31-1 queries)");
  *npairs = 0;
  if (nq == 0) return 0;
  if (!qptr) return fail("qptr is null");
  if (qptr[0] != 0) return fail("qptr[0] must be 0");
  for (int64_t q = 0; q < nq; ++q)
    if (qptr[q + 1] < qptr[q]) return fail("qptr not monotone");
  const int64_t np = qptr[nq], nother = c->s[1 - side].n;
  if (np > 0 && !targets) return fail("targets is null");
  for (int64_t p = 0; p < np; ++p)
    if (targets[p] < 0 || targets[p] >= nother) return fail("target out of range");
  *npairs = np;
  return 0;
}

// Uploads the queries, runs the kernel and copies the answers out.  h_rowptr / d_rowptr: the
// explained rows' CSR offsets on the host and the device; d_col / d_val are indexed with them.
// rows = nullptr: query q is row q.
int explain_run(qmfx_ctx* c, int side, int64_t nq, const int64_t* rows, const int64_t* h_rowptr,
                const int64_t* d_rowptr, const int32_t* d_col, const void* d_val,
                const int64_t* qptr, const int64_t* targets, int64_t npairs, double alpha,
                double lambda, int topm, const Outputs& o) {
  if (!o.sources || !o.positions || !o.contribs || !o.counts || !o.totals)
    return fail("sources, positions, contribs, counts or totals is null");
  const SideBuf& R = c->s[1 - side];
  const size_t nq1 = (size_t)nq, np = (size_t)npairs, lists = np * (size_t)topm;
  // the full vector's layout, and the work counted for the call
  std::vector<int64_t> allq(nq1);
  int64_t nall = 0;
  double nz_sys = 0, nz_pairs = 0, nsys = 0;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t r = rows ? rows[q] : q, n = h_rowptr[r + 1] - h_rowptr[r];
    const int64_t t = qptr[q + 1] - qptr[q];
    allq[q] = nall;
    nall += t * n;
    if (t > 0) {
      nsys += 1;
      nz_sys += (double)n;
      nz_pairs += (double)t * (double)n;
    }
  }
  const bool in_lds = c->kp <= kExplainLdsMaxKP;
  const size_t tri = (size_t)c->kp * (c->kp + 1) / 2;
  if (rows)
    if (int rc = reserve(c->ex_rows, nq1 * 8)) return rc;
  if (int rc = reserve(c->ex_qptr, (nq1 + 1) * 8)) return rc;
  if (int rc = reserve(c->ex_targets, np * 8)) return rc;
  if (o.all)
    if (int rc = reserve(c->ex_allq, nq1 * 8)) return rc;
  if (int rc = reserve(c->ex_sources, lists * 8)) return rc;
  if (int rc = reserve(c->ex_positions, lists * 8)) return rc;
  if (int rc = reserve(c->ex_contribs, lists * 8)) return rc;
  if (int rc = reserve(c->ex_totals, np * 8)) return rc;
  if (o.all && nall > 0)
    if (int rc = reserve(c->ex_all, (size_t)nall * 8)) return rc;
  if (!in_lds)
    if (int rc = reserve(c->ex_scratch, (size_t)explain_grid(nq, c->kp) * tri * 8))
      return rc;
  if (int rc = reserve(c->ex_counts, np * 4)) return rc;
  if (int rc = reserve(c->ex_first, 8)) return rc;
  if (rows) HIPCHK(scopy(c, c->ex_rows, rows, nq1 * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, c->ex_qptr, qptr, (nq1 + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, c->ex_targets, targets, np * 8, hipMemcpyHostToDevice));
  if (o.all) HIPCHK(scopy(c, c->ex_allq, allq.data(), nq1 * 8, hipMemcpyHostToDevice));
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  HIPCHK(hipMemsetAsync(c->ex_first, 0xff, 8, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    // YᵀY of the other side's current factors, computed by every call
    HIPCHK(launch_gram_t<T>(c, R));
    ExplainArgs<T> a{};
    a.sys.col = d_col;
    a.sys.val = static_cast<const T*>(d_val);
    a.sys.Y = R.F.as<T>();
    a.sys.G = c->G.as<T>();
    a.sys.alpha = alpha;
    a.sys.lambda = lambda;
    a.sys.k = c->k;
    a.sys.kp = c->kp;
    a.sys.scratch = c->ex_scratch;
    a.rowptr = d_rowptr;
    a.rows = rows ? c->ex_rows.get() : nullptr;
    a.nq = nq;
    a.qptr = c->ex_qptr;
    a.targets = c->ex_targets;
    a.topm = topm;
    a.sources = c->ex_sources;
    a.positions = c->ex_positions;
    a.contribs = c->ex_contribs;
    a.counts = c->ex_counts;
    a.totals = c->ex_totals;
    a.all = o.all && nall > 0 ? c->ex_all.get() : nullptr;
    a.allq = c->ex_allq;
    a.first_bad = c->ex_first;
    const hipError_t e = launch_explain(a, c->stream);
    if (e != hipSuccess) return fail(std::string("explain kernel launch: ") + hipGetErrorString(e), -2);
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  unsigned long long first = 0;
  HIPCHK(scopy(c, &first, c->ex_first, 8, hipMemcpyDeviceToHost));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  // the work formula of include/qmfx.h
  const double k = c->k, s = (double)c->esz;
  c->solve.add(ms, nz_sys * k * (k + 1) + nsys * k * k * k / 3.0 + (double)npairs * 2 * k * k +
                       nz_pairs * 2 * k,
               nz_sys * (4 + s + k * s) + (double)npairs * k * s + nz_pairs * k * s +
                       (double)lists * 24 + (double)npairs * 12 + (o.all ? (double)nall * 8 : 0.0));
  if (first != ~0ull)
    return fail("the row system of query " + std::to_string(first) +
                    " is not positive definite (some 1 + αv < 0, or λ ≤ 0): explanations are "
                    "defined for positive definite systems only",
                -5);
  HIPCHK(scopy(c, o.sources, c->ex_sources, lists * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, o.positions, c->ex_positions, lists * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, o.contribs, c->ex_contribs, lists * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, o.counts, c->ex_counts, np * 4, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, o.totals, c->ex_totals, np * 8, hipMemcpyDeviceToHost));
  if (o.all && nall > 0) HIPCHK(scopy(c, o.all, c->ex_all, (size_t)nall * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int qmfx_wals_explain(qmfx_ctx* c, int side, int64_t nq, const int64_t* rows, const int64_t* qptr,
                      const int64_t* targets, double alpha, double lambda, int topm,
                      int64_t* sources, int64_t* positions, double* contribs, int32_t* counts,
                      double* totals, double* all) {
  int64_t npairs = 0;
  if (int rc = explain_checks(c, side, nq, qptr, targets, topm, &npairs)) return rc;
  const SideBuf& L = c->s[side];
  if (!L.rowptr) return fail("no interactions uploaded for this side");
  if (nq > 0 && !rows) return fail("rows is null");
  for (int64_t q = 0; q < nq; ++q) {
    if (rows[q] < 0 || rows[q] >= L.n) return fail("row out of range");
    if (L.sharded && (rows[q] < L.rbeg || rows[q] >= L.rend))
      return fail("row not held by this rank");
  }
  if (npairs == 0) return 0;
  if (set_dev(c)) return -2;
  const void* val = c->prec == 32 ? (const void*)valp<float>(L) : (const void*)valp<double>(L);
  return explain_run(c, side, nq, rows, L.h_rowptr.data(), L.rowptr, colp(L), val, qptr, targets,
                     npairs, alpha, lambda, topm,
                     Outputs{sources, positions, contribs, counts, totals, all});
}

int qmfx_wals_explain_rows(qmfx_ctx* c, int side, int64_t nrows, const int64_t* rowptr,
                           const int32_t* colidx, const double* values, const int64_t* qptr,
                           const int64_t* targets, double alpha, double lambda, int topm,
                           int64_t* sources, int64_t* positions, double* contribs,
                           int32_t* counts, double* totals, double* all) {
  int64_t npairs = 0, max_n = 0;
  if (int rc = explain_checks(c, side, nrows, qptr, targets, topm, &npairs)) return rc;
  if (int rc = validate_rows(nrows, rowptr, colidx, values, c->s[1 - side].n, false, &max_n))
    return rc;
  if (npairs == 0) return 0;
  if (set_dev(c)) return -2;
  if (int rc = upload_rows(c, nrows, rowptr, colidx, values)) return rc;
  return explain_run(c, side, nrows, nullptr, rowptr, c->fr_rowptr, c->fr_col, c->fr_val, qptr,
                     targets, npairs, alpha, lambda, topm,
                     Outputs{sources, positions, contribs, counts, totals, all});
}

int qmfx_row_lengths(qmfx_ctx* c, int side, int64_t n, const int64_t* rows, int64_t* lengths) {
  if (!c) return fail("null context");
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  const SideBuf& L = c->s[side];
  if (!L.rowptr) return fail("no interactions uploaded for this side");
  for (int64_t i = 0; i < n; ++i) {
    if (rows[i] < 0 || rows[i] >= L.n) return fail("row out of range");
    lengths[i] = L.h_rowptr[rows[i] + 1] - L.h_rowptr[rows[i]];
  }
  return 0;
}

}  // extern "C"
