// Top-N recommendations: the requested users' best eligible items, selected on the device.
#include "ctx.h"

using namespace qmfx;

extern "C" {

int qmfx_recommend(qmfx_ctx* c, int64_t nusers, const int64_t* users, int topn, int exclude,
                   int use_biases, int64_t* items, double* scores, int32_t* counts) {
  if (nusers == 0) return 0;
  if (nusers < 0) return fail("nusers out of range");
  if (topn < 1 || topn > QMFX_REC_MAX_N) return fail("topn must be in 1..128 (QMFX_REC_MAX_N)");
  if (exclude != QMFX_REC_ALL && exclude != QMFX_REC_UNSEEN_SIGNALS &&
      exclude != QMFX_REC_UNSEEN_POSITIVES)
    return fail("unknown exclude mode");
  if (!c->s[0].F || !c->s[1].F) return fail("factors not allocated (qmfx_set_shape first)");
  if (c->k > 256) return fail("recommendations support nfactors <= 256");
  if (use_biases && !c->bias) return fail("no item biases on the context");
  const SideBuf& su = c->s[0];
  if (exclude == QMFX_REC_UNSEEN_SIGNALS && (!su.rowptr || !su.col))
    return fail("no user signals on the context (QMFX_REC_UNSEEN_SIGNALS needs the side-0 CSR)");
  if (exclude == QMFX_REC_UNSEEN_POSITIVES && (!c->urowptr || !c->uitems))
    return fail("no positives on the context (QMFX_REC_UNSEEN_POSITIVES needs "
                "qmfx_bpr_set_positives)");
  // a sharded context holds only its own rows' signals
  const bool own_rows = exclude == QMFX_REC_UNSEEN_SIGNALS && su.sharded;
  for (int64_t t = 0; t < nusers; ++t) {
    if (users[t] < 0 || users[t] >= su.n) return fail("user index out of range");
    if (own_rows && (users[t] < su.rbeg || users[t] >= su.rend))
      return fail("user not held by this rank (QMFX_REC_UNSEEN_SIGNALS on a sharded context)");
  }
  if (set_dev(c)) return -2;

  const int64_t ni = c->s[1].n;
  if (int rc = topn_reserve(c, nusers, ni, topn)) return rc;
  HIPCHK(scopy(c, c->rc.users, users, (size_t)nusers * 8, hipMemcpyHostToDevice));

  HIPCHK(hipEventRecord(c->ev0, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    RecArgs<T> a{};
    topn_args(c, a, nusers, ni, topn);
    a.U = c->s[0].F.as<T>();
    a.I = c->s[1].F.as<T>();
    a.bias = use_biases ? c->bias.as<T>() : nullptr;
    if (exclude == QMFX_REC_UNSEEN_SIGNALS) {
      a.seen_ptr = su.rowptr;
      a.seen_col = colp(su);
    } else if (exclude == QMFX_REC_UNSEEN_POSITIVES) {
      a.seen_ptr = c->urowptr;
      a.seen_col = c->uitems;
    }
    HIPCHK(launch_recommend(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  if (int r = topn_copy_out(c, nusers, topn, items, scores, counts)) return r;
  // the call's kernels, for qmfx_solve_kernel_stats
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->solve.add(ms, topn_flops(c, nusers, ni), topn_bytes(c, nusers, ni));
  return 0;
}

}  // extern "C"
