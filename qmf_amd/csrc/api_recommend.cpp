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
  const size_t lists = (size_t)(eval_chunks(nusers, ni) * eval_user_rows(nusers));
  const size_t out = (size_t)nusers * (size_t)topn;
  if (int rc = grow(c->rc_users, c->rc_cap[0], (size_t)nusers * 8)) return rc;
  if (int rc = grow(c->rc_items, c->rc_cap[1], out * 8)) return rc;
  if (int rc = grow(c->rc_udbl, c->rc_cap[2], (size_t)(eval_user_rows(nusers) * c->k) * 8)) return rc;
  if (int rc = grow(c->rc_pscore, c->rc_cap[3], lists * (size_t)topn * 8)) return rc;
  if (int rc = grow(c->rc_scores, c->rc_cap[4], out * 8)) return rc;
  if (int rc = grow(c->rc_pitem, c->rc_cap[5], lists * (size_t)topn * 4)) return rc;
  if (int rc = grow(c->rc_pcnt, c->rc_cap[6], lists * 4)) return rc;
  if (int rc = grow(c->rc_counts, c->rc_cap[7], (size_t)nusers * 4)) return rc;
  HIPCHK(scopy(c, c->rc_users, users, (size_t)nusers * 8, hipMemcpyHostToDevice));

  HIPCHK(hipEventRecord(c->ev0, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    RecArgs<T> a{};
    a.U = c->s[0].F.as<T>();
    a.I = c->s[1].F.as<T>();
    a.bias = use_biases ? c->bias.as<T>() : nullptr;
    a.users = c->rc_users;
    a.nreq = nusers;
    a.nitems = ni;
    a.k = c->k;
    a.kp = c->kp;
    a.topn = topn;
    if (exclude == QMFX_REC_UNSEEN_SIGNALS) {
      a.seen_ptr = su.rowptr;
      a.seen_col = colp(su);
    } else if (exclude == QMFX_REC_UNSEEN_POSITIVES) {
      a.seen_ptr = c->urowptr;
      a.seen_col = c->uitems;
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
  HIPCHK(scopy(c, items, c->rc_items, out * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, scores, c->rc_scores, out * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, counts, c->rc_counts, (size_t)nusers * 4, hipMemcpyDeviceToHost));
  // the call's kernels, for qmfx_solve_kernel_stats (one unit = one user × item score: 2k
  // flop; bytes: the item factors once per group of 32 users)
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->solve.add(ms, 2.0 * (double)nusers * (double)ni * c->k,
               (double)((nusers + 31) / 32) * (double)ni * c->k * (double)c->esz);
  return 0;
}

}  // extern "C"
