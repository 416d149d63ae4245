// Top-N recommendations: the requested users' best eligible items, selected on the device;
// over the whole catalogue (qmfx_recommend), without a deny list's items
// (qmfx_recommend_without), or within candidate lists (qmfx_recommend_candidates).
#include "ctx.h"

using namespace qmfx;

namespace qmfx {

// What every recommend call rejects before it touches the device.
int rec_check(const qmfx_ctx* c, int64_t nusers, const int64_t* users, int topn, int exclude,
              int use_biases) {
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
  return 0;
}

}  // namespace qmfx

namespace {

// The call's kernels (between ev0 and ev1), for qmfx_solve_kernel_stats.
int rec_account(qmfx_ctx* c, double flops, double bytes) {
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->solve.add(ms, flops, bytes);
  return 0;
}

}  // namespace

// qmfx_recommend, with the ndeny items of `deny` eligible for nobody.
int qmfx::recommend_dense(qmfx_ctx* c, int64_t nusers, const int64_t* users, int64_t ndeny,
                          const int64_t* deny, int topn, int exclude, int use_biases,
                          int64_t* items, double* scores, int32_t* counts) {
  if (nusers == 0) return 0;
  if (ndeny < 0) return fail("ndeny out of range");
  if (int rc = rec_check(c, nusers, users, topn, exclude, use_biases)) return rc;
  const int64_t ni = c->s[1].n;
  std::vector<unsigned long long> bits;
  if (ndeny > 0) {
    bits.assign((size_t)((ni + 63) / 64), 0ull);
    for (int64_t j = 0; j < ndeny; ++j) {
      if (deny[j] < 0 || deny[j] >= ni) return fail("deny item index out of range");
      bits[(size_t)(deny[j] >> 6)] |= 1ull << (deny[j] & 63);
    }
  }
  if (set_dev(c)) return -2;

  if (int rc = topn_reserve(c, nusers, ni, topn)) return rc;
  HIPCHK(scopy(c, c->rc.users, users, (size_t)nusers * 8, hipMemcpyHostToDevice));
  if (ndeny > 0) {
    if (int rc = reserve(c->rc.deny, bits.size() * 8)) return rc;
    HIPCHK(scopy(c, c->rc.deny, bits.data(), bits.size() * 8, hipMemcpyHostToDevice));
  }

  HIPCHK(hipEventRecord(c->ev0, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    RecArgs<T> a{};
    topn_args(c, a, nusers, ni, topn);
    rec_model(c, a, exclude, use_biases);
    a.deny = ndeny > 0 ? c->rc.deny.get() : nullptr;
    HIPCHK(launch_recommend(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  if (int r = topn_copy_out(c, nusers, topn, items, scores, counts)) return r;
  return rec_account(c, topn_flops(c, nusers, ni), topn_bytes(c, nusers, ni));
}

namespace {

// cand[b .. e) as int32 into out: strictly ascending item rows
int take_list(const int64_t* cand, int64_t b, int64_t e, int64_t ni, int32_t* out) {
  for (int64_t j = b; j < e; ++j) {
    if (cand[j] < 0 || cand[j] >= ni) return fail("candidate item index out of range");
    if (j > b && cand[j] <= cand[j - 1])
      return fail("a candidate list is not strictly ascending");
    out[j] = (int32_t)cand[j];
  }
  return 0;
}

}  // namespace

extern "C" {

int qmfx_recommend(qmfx_ctx* c, int64_t nusers, const int64_t* users, int topn, int exclude,
                   int use_biases, int64_t* items, double* scores, int32_t* counts) {
  return recommend_dense(c, nusers, users, 0, nullptr, topn, exclude, use_biases, items, scores,
                         counts);
}

int qmfx_recommend_without(qmfx_ctx* c, int64_t nusers, const int64_t* users, int64_t ndeny,
                           const int64_t* deny, int topn, int exclude, int use_biases,
                           int64_t* items, double* scores, int32_t* counts) {
  return recommend_dense(c, nusers, users, ndeny, deny, topn, exclude, use_biases, items, scores,
                         counts);
}

int qmfx_recommend_candidates(qmfx_ctx* c, int64_t nusers, const int64_t* users,
                              const int64_t* cptr, int64_t ncand, const int64_t* cand, int topn,
                              int exclude, int use_biases, int64_t* items, double* scores,
                              int32_t* counts) {
  if (nusers == 0) return 0;
  if (int rc = rec_check(c, nusers, users, topn, exclude, use_biases)) return rc;
  const bool shared = cptr == nullptr;
  if (shared && ncand < 0) return fail("ncand out of range");
  if (!shared) {
    if (cptr[0] != 0) return fail("cptr[0] must be 0");
    for (int64_t t = 0; t < nusers; ++t)
      if (cptr[t + 1] < cptr[t]) return fail("cptr is decreasing");
  }
  const int64_t total = shared ? ncand : cptr[nusers];
  if (total >= (int64_t)1 << 31) return fail("2^31 candidates or more");
  if (nusers >= (int64_t)1 << 31) return fail("2^31 users or more");
  const int64_t ni = c->s[1].n;
  // the lists as int32 rows; per-user form: user t's chunks are the work items
  // woff[t] .. woff[t + 1], and wuser names a work item's user
  std::vector<int32_t> h_cand((size_t)total), wuser;
  std::vector<int64_t> woff;
  double pairs = 0;  // Σ (user, candidate)
  if (shared) {
    if (int rc = take_list(cand, 0, ncand, ni, h_cand.data())) return rc;
    pairs = (double)nusers * (double)ncand;
  } else {
    woff.assign((size_t)nusers + 1, 0);
    for (int64_t t = 0; t < nusers; ++t) {
      if (int rc = take_list(cand, cptr[t], cptr[t + 1], ni, h_cand.data())) return rc;
      woff[t + 1] = woff[t] + cand_chunks(cptr[t + 1] - cptr[t]);
    }
    wuser.resize((size_t)woff[nusers]);
    for (int64_t t = 0; t < nusers; ++t)
      std::fill(wuser.begin() + woff[t], wuser.begin() + woff[t + 1], (int32_t)t);
    pairs = (double)total;
  }
  if (set_dev(c)) return -2;

  TopN& s = c->rc;
  const size_t lists = shared ? (size_t)(cand_chunks(ncand) * eval_user_rows(nusers))
                              : (size_t)woff[nusers];
  if (int rc = topn_reserve_lists(c, nusers, lists, topn)) return rc;
  if (int rc = reserve(s.cand, h_cand.size() * 4)) return rc;
  HIPCHK(scopy(c, s.users, users, (size_t)nusers * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, s.cand, h_cand.data(), h_cand.size() * 4, hipMemcpyHostToDevice));
  if (!shared) {
    const size_t np = ((size_t)nusers + 1) * 8;
    if (int rc = reserve(s.cptr, np)) return rc;
    if (int rc = reserve(s.woff, np)) return rc;
    if (int rc = reserve(s.wuser, wuser.size() * 4)) return rc;
    HIPCHK(scopy(c, s.cptr, cptr, np, hipMemcpyHostToDevice));
    HIPCHK(scopy(c, s.woff, woff.data(), np, hipMemcpyHostToDevice));
    HIPCHK(scopy(c, s.wuser, wuser.data(), wuser.size() * 4, hipMemcpyHostToDevice));
  }

  HIPCHK(hipEventRecord(c->ev0, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    CandArgs<T> a{};
    topn_args(c, a, nusers, ni, topn);
    rec_model(c, a, exclude, use_biases);
    a.cand = s.cand;
    a.ncand = shared ? ncand : 0;
    if (!shared) {
      a.cptr = s.cptr;
      a.woff = s.woff;
      a.wuser = s.wuser;
      a.h_woff = woff.data();
    }
    HIPCHK(launch_recommend_candidates(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  if (int r = topn_copy_out(c, nusers, topn, items, scores, counts)) return r;
  // 2k flop per (user, candidate) pair; the gathered rows once per workgroup
  const double rows = shared ? (double)((nusers + 31) / 32) * (double)ncand : pairs;
  return rec_account(c, 2.0 * pairs * c->k, rows * c->k * (double)c->esz);
}

}  // extern "C"
