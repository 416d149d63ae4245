// Test-set evaluation: the labelled pairs of the test users and their ranking statistics.
#include "ctx.h"

using namespace qmfx;

template <typename T>
static EvalArgs<T> eval_args(qmfx_ctx* c, int use_biases) {
  EvalArgs<T> a{};
  a.U = c->s[0].F.as<T>();
  a.I = c->s[1].F.as<T>();
  a.bias = use_biases ? c->bias.as<T>() : nullptr;
  a.users = c->ev_users;
  a.ntest = c->ev_ntest;
  a.nitems = c->s[1].n;
  a.k = c->k;
  a.kp = c->kp;
  a.lab_slot = c->ev_slot;
  a.lab_item = c->ev_item;
  a.lab_pidx = c->ev_pidx;
  a.nlab = c->ev_nlab;
  a.lab_score = c->ev_lscore;
  a.pptr = c->ev_pptr;
  a.pscore = c->ev_pscore;
  a.above = c->ev_above;
  a.sq_part = c->ev_sq;
  a.udbl = c->ev_udbl;
  return a;
}

// The label set indexes both sides' rows, and ev_sq / ev_chunks are sized from the item count:
// a new label set and a changed shape (qmfx_set_shape) both start from none.
void qmfx::drop_eval_labels(qmfx_ctx* c) {
  c->ev_users.reset();
  c->ev_slot.reset();
  c->ev_item.reset();
  c->ev_pidx.reset();
  c->ev_pptr.reset();
  c->ev_lscore.reset();
  c->ev_pscore.reset();
  c->ev_above.reset();
  c->ev_sq.reset();
  c->ev_udbl.reset();
  c->ev_ntest = c->ev_nlab = c->ev_npos = c->ev_chunks = 0;
}

extern "C" {

int qmfx_eval_set_labels(qmfx_ctx* c, int64_t ntest, const int64_t* users, const int64_t* rowptr,
                         const int64_t* items, const double* values) {
  if (!c->s[0].F || !c->s[1].F) return fail("factors not allocated (qmfx_set_shape first)");
  if (ntest < 0) return fail("ntest out of range");
  if (c->k > 256) return fail("evaluation supports nfactors <= 256");
  if (set_dev(c)) return -2;
  const int64_t nu = c->s[0].n, ni = c->s[1].n;
  if (ntest > 0 && rowptr[0] != 0) return fail("label rowptr must start at 0");
  const int64_t nlab = ntest > 0 ? rowptr[ntest] : 0;
  std::vector<int32_t> slot((size_t)nlab);
  std::vector<int64_t> pidx((size_t)nlab), pptr((size_t)ntest + 1, 0);
  int64_t np = 0;
  for (int64_t t = 0; t < ntest; ++t) {
    if (users[t] < 0 || users[t] >= nu) return fail("test user index out of range");
    if (rowptr[t + 1] < rowptr[t]) return fail("label rowptr not ascending");
    pptr[(size_t)t] = np;
    for (int64_t e = rowptr[t]; e < rowptr[t + 1]; ++e) {
      if (items[e] < 0 || items[e] >= ni) return fail("label item index out of range");
      slot[(size_t)e] = (int32_t)t;
      pidx[(size_t)e] = values[e] > 0.0 ? np++ : -1;
    }
  }
  pptr[(size_t)ntest] = np;
  const int64_t nch = eval_chunks(ntest, ni);
  // the previous label set goes before the new one is allocated
  drop_eval_labels(c);
  const size_t nl = (size_t)std::max<int64_t>(nlab, 1), npp = (size_t)std::max<int64_t>(np, 1);
  HIPCHK(dev_alloc(c->ev_users, (size_t)std::max<int64_t>(ntest, 1) * 8));
  HIPCHK(dev_alloc(c->ev_slot, nl * 4));
  HIPCHK(dev_alloc(c->ev_item, nl * 8));
  HIPCHK(dev_alloc(c->ev_pidx, nl * 8));
  HIPCHK(dev_alloc(c->ev_pptr, ((size_t)ntest + 1) * 8));
  HIPCHK(dev_alloc(c->ev_lscore, nl * 8));
  HIPCHK(dev_alloc(c->ev_pscore, npp * 8));
  HIPCHK(dev_alloc(c->ev_above, npp * 8));
  HIPCHK(dev_alloc(c->ev_sq, (size_t)std::max<int64_t>(nch * ntest, 1) * 8));
  HIPCHK(dev_alloc(c->ev_udbl, (size_t)std::max<int64_t>(eval_user_rows(ntest) * c->k, 1) * 8));
  HIPCHK(scopy(c, c->ev_users, users, (size_t)ntest * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, c->ev_slot, slot.data(), (size_t)nlab * 4, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, c->ev_item, items, (size_t)nlab * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, c->ev_pidx, pidx.data(), (size_t)nlab * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, c->ev_pptr, pptr.data(), pptr.size() * 8, hipMemcpyHostToDevice));
  c->ev_ntest = ntest;
  c->ev_nlab = nlab;
  c->ev_npos = np;
  c->ev_chunks = nch;
  return 0;
}

int qmfx_eval_ranks(qmfx_ctx* c, int use_biases, double* label_scores, int64_t* above,
                    double* sq_sum) {
  if (!c->ev_users) return fail("no test labels (qmfx_eval_set_labels first)");
  if (use_biases && !c->bias) return fail("no item biases on the context");
  if (set_dev(c)) return -2;
  const int64_t nt = c->ev_ntest, nch = c->ev_chunks;
  HIPCHK(hipMemsetAsync(c->ev_above, 0, (size_t)std::max<int64_t>(c->ev_npos, 1) * 8, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    HIPCHK(launch_eval_ranks(eval_args<decltype(t)>(c, use_biases), c->stream));
    return 0;
  });
  if (rc) return rc;
  std::vector<double> part((size_t)(nch * nt));
  HIPCHK(scopy(c, label_scores, c->ev_lscore, (size_t)c->ev_nlab * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, above, c->ev_above, (size_t)c->ev_npos * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, part.data(), c->ev_sq, part.size() * 8, hipMemcpyDeviceToHost));
  for (int64_t t = 0; t < nt; ++t) {
    double v = 0.0;
    for (int64_t ch = 0; ch < nch; ++ch) v += part[(size_t)(ch * nt + t)];
    sq_sum[t] = v;
  }
  return 0;
}

}  // extern "C"
