// Similar rows: the top-N neighbours of a side's rows among the rows of the same side, by dot
// product or cosine, selected on the device (qmfx_similar), and the row norms the cosine uses
// (qmfx_factor_norms).
#include "ctx.h"

using namespace qmfx;

namespace {

// the side's norms into c->sim_norms (recomputed by every call: any write to the factors
// would have to invalidate a cached copy, and the pass costs about one query)
int compute_norms(qmfx_ctx* c, int side) {
  const SideBuf& sb = c->s[side];
  if (int rc = reserve(c->sim_norms, (size_t)sb.n * 8)) return rc;
  return with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    HIPCHK(launch_factor_norms(sb.F.as<T>(), sb.n, c->k, c->kp, c->sim_norms, c->stream));
    return 0;
  });
}

}  // namespace

extern "C" {

int qmfx_factor_norms(qmfx_ctx* c, int side, double* norms) {
  if (side != 0 && side != 1) return fail("side must be 0 (users) or 1 (items)");
  if (!c->s[side].F) return fail("factors not allocated (qmfx_set_shape first)");
  if (set_dev(c)) return -2;
  if (int rc = compute_norms(c, side)) return rc;
  HIPCHK(scopy(c, norms, c->sim_norms, (size_t)c->s[side].n * 8, hipMemcpyDeviceToHost));
  return 0;
}

int qmfx_similar(qmfx_ctx* c, int side, int64_t nq, const int64_t* rows, int topn, int metric,
                 int exclude_self, int64_t* neighbours, double* scores, int32_t* counts) {
  if (side != 0 && side != 1) return fail("side must be 0 (users) or 1 (items)");
  if (nq == 0) return 0;
  if (nq < 0) return fail("nq out of range");
  if (topn < 1 || topn > QMFX_REC_MAX_N) return fail("topn must be in 1..128 (QMFX_REC_MAX_N)");
  if (metric != QMFX_SIM_DOT && metric != QMFX_SIM_COSINE) return fail("unknown similarity metric");
  const SideBuf& sb = c->s[side];
  if (!sb.F) return fail("factors not allocated (qmfx_set_shape first)");
  if (c->k > 256) return fail("similar rows support nfactors <= 256");
  for (int64_t t = 0; t < nq; ++t)
    if (rows[t] < 0 || rows[t] >= sb.n) return fail("row index out of range");
  if (set_dev(c)) return -2;

  if (int rc = topn_reserve(c, nq, sb.n, topn)) return rc;
  HIPCHK(scopy(c, c->rc.users, rows, (size_t)nq * 8, hipMemcpyHostToDevice));

  HIPCHK(hipEventRecord(c->ev0, c->stream));
  if (metric == QMFX_SIM_COSINE)
    if (int rc = compute_norms(c, side)) return rc;
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    SimArgs<T> a{};
    topn_args(c, a, nq, sb.n, topn);
    a.U = sb.F.as<T>();
    a.I = sb.F.as<T>();
    a.norms = c->sim_norms;
    a.cosine = metric == QMFX_SIM_COSINE;
    a.exclude_self = exclude_self != 0;
    HIPCHK(launch_similar(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  if (int r = topn_copy_out(c, nq, topn, neighbours, scores, counts)) return r;
  // the call's kernels, for qmfx_solve_kernel_stats
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->solve.add(ms, topn_flops(c, nq, sb.n), topn_bytes(c, nq, sb.n));
  return 0;
}

}  // extern "C"
