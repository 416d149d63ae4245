// BPR: positives, item biases, the Hogwild epoch, and the serial update / loss evaluation
// over explicit triplets.
#include "ctx.h"

using namespace qmfx;

namespace {

uint64_t gcd64(uint64_t a, uint64_t b) {
  while (b) {
    uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

template <typename T>
BprArgs<T> bpr_args(qmfx_ctx* c, double lr, double bl, double ul, double il, int ub) {
  BprArgs<T> a{};
  a.U = c->s[0].F.as<T>();
  a.I = c->s[1].F.as<T>();
  a.bias = c->bias.as<T>();
  a.pos_user = c->pos_user;
  a.pos_item = c->pos_item;
  a.npos = c->npos;
  a.urowptr = c->urowptr;
  a.uitems = c->uitems;
  a.nitems = c->s[1].n;
  a.lr = (T)lr;
  a.bias_lambda = (T)bl;
  a.user_lambda = (T)ul;
  a.item_lambda = (T)il;
  a.use_biases = ub;
  a.kp = c->kp;
  a.bad = c->bad;
  // Hogwild width: concurrent waves that touch the same user or item row read it stale (row
  // changes are added atomically, so no update is lost).  Keep the expected number of
  // concurrent waves per row small: ≈ min(nusers, nitems)/16 waves, capped at 16 waves per
  // CU (4096), at least 1 (a 3-user problem runs serially, as the reference's 1-thread
  // default does).
  const int64_t rows = std::min(c->s[0].n, c->s[1].n);
  a.waves = (int)std::max<int64_t>(1, std::min<int64_t>({4096, rows / 16, std::max<int64_t>(c->npos, 1)}));
  // The user row is stored plainly (an overwrite is the reference's Hogwild store) only while
  // two waves rarely hold the same user: the heaviest user's share of the positives times
  // the concurrent waves is the chance that another wave holds that user at a given moment.
  // Above 1% (skewed user activity) its net change is added atomically like the item rows.
  a.atomic_user = (double)a.waves * (double)c->max_user_pos > 0.01 * (double)std::max<int64_t>(c->npos, 1) ? 1 : 0;
  if (const char* f = std::getenv("QMFX_BPR_ATOMIC_USER")) a.atomic_user = std::atoi(f) ? 1 : 0;
  // 4097 rejections in a row have probability (positives/nitems)^4097 per draw: below 1e-35
  // under 98% of the items, so only heavier users get the kernel that handles a capped draw
  a.capped = (double)c->max_user_pos >= 0.98 * (double)c->s[1].n ? 1 : 0;
  return a;
}

// every index of the n (user, positive item, negative item) triplets within the shape
bool triplets_in_range(const qmfx_ctx* c, const int64_t* trip, int64_t n) {
  for (int64_t t = 0; t < n; ++t)
    if (trip[3 * t] < 0 || trip[3 * t] >= c->s[0].n || trip[3 * t + 1] < 0 ||
        trip[3 * t + 1] >= c->s[1].n || trip[3 * t + 2] < 0 || trip[3 * t + 2] >= c->s[1].n)
      return false;
  return true;
}

}  // namespace

const char* const qmfx::kBadGradients =
    "gradients too big, try decreasing the learning rate (--init_learning_rate)";

// The positives index both sides' rows and urowptr is sized from the user count; the cached
// triplets of qmfx_bpr_eval were range-checked against the shape they were uploaded under.
void qmfx::drop_bpr_positives(qmfx_ctx* c) {
  c->pos_user.reset();
  c->pos_item.reset();
  c->urowptr.reset();
  c->uitems.reset();
  c->npos = 0;
  c->max_user_pos = 0;
  for (int slot = 0; slot < 2; ++slot) {
    c->trip[slot].reset();
    c->trip_src[slot] = nullptr;
    c->trip_n[slot] = 0;
  }
}

extern "C" {

int qmfx_bpr_set_positives(qmfx_ctx* c, const int64_t* users, const int64_t* items, int64_t npos) {
  const int64_t nu = c->s[0].n, ni = c->s[1].n;
  if (nu <= 0 || ni <= 0) return fail("shape not set (qmfx_set_shape)");
  if (set_dev(c)) return -2;
  std::vector<int32_t> it((size_t)std::max<int64_t>(npos, 1));
  for (int64_t e = 0; e < npos; ++e) {
    if (users[e] < 0 || users[e] >= nu || items[e] < 0 || items[e] >= ni)
      return fail("positive index out of range");
    it[e] = (int32_t)items[e];
  }
  c->pos_item.reset();
  c->urowptr.reset();
  c->uitems.reset();
  HIPCHK(dev_alloc(c->pos_user, (size_t)std::max<int64_t>(npos, 1) * 8));
  HIPCHK(dev_alloc(c->pos_item, (size_t)std::max<int64_t>(npos, 1) * 4));
  if (npos > 0) {
    HIPCHK(scopy(c, c->pos_user, users, (size_t)npos * 8, hipMemcpyHostToDevice));
    HIPCHK(scopy(c, c->pos_item, it.data(), (size_t)npos * 4, hipMemcpyHostToDevice));
  }
  // per-user sorted positive items (the reference's itemMap_, BPREngine.cpp:79-82)
  std::vector<uint64_t> keys((size_t)npos);
  for (int64_t e = 0; e < npos; ++e) keys[e] = (uint64_t)users[e] * (uint64_t)ni + (uint64_t)items[e];
  std::sort(keys.begin(), keys.end());
  std::vector<int64_t> rp((size_t)nu + 1, 0);
  std::vector<int32_t> ui((size_t)std::max<int64_t>(npos, 1));
  for (int64_t e = 0; e < npos; ++e) {
    rp[keys[e] / ni + 1]++;
    ui[e] = (int32_t)(keys[e] % ni);
  }
  c->max_user_pos = 0;
  for (int64_t u = 0; u < nu; ++u) c->max_user_pos = std::max(c->max_user_pos, rp[u + 1]);
  for (int64_t u = 0; u < nu; ++u) rp[u + 1] += rp[u];
  HIPCHK(dev_alloc(c->urowptr, (size_t)(nu + 1) * 8));
  HIPCHK(dev_alloc(c->uitems, ui.size() * 4));
  HIPCHK(scopy(c, c->urowptr, rp.data(), rp.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, c->uitems, ui.data(), ui.size() * 4, hipMemcpyHostToDevice));
  c->npos = npos;
  if (int rc = ensure_side_factors(c, 0)) return rc;
  if (int rc = ensure_side_factors(c, 1)) return rc;
  return ensure_bias(c);
}

int qmfx_bpr_set_biases(qmfx_ctx* c, const double* bias) {
  const int64_t ni = c->s[1].n;
  if (ni <= 0) return fail("shape not set");
  if (set_dev(c)) return -2;
  if (!c->bias) HIPCHK(dev_alloc(c->bias, (size_t)ni * c->esz));
  HIPCHK(copy_in(c, c->bias, bias, (size_t)ni));
  return 0;
}

int qmfx_bpr_get_biases(qmfx_ctx* c, double* bias) {
  const int64_t ni = c->s[1].n;
  if (!c->bias) return fail("no biases");
  if (set_dev(c)) return -2;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(copy_out(c, bias, c->bias, (size_t)ni));
  return 0;
}

int qmfx_bpr_epoch(qmfx_ctx* c, uint64_t seed, int num_neg, double lr, double bias_lambda,
                   double user_lambda, double item_lambda, int use_biases, int shuffle) {
  if (!c->pos_user) return fail("no positives (qmfx_bpr_set_positives)");
  if (c->npos == 0) return 0;
  if (set_dev(c)) return -2;
  uint64_t pa = 1, pb = 0;
  if (shuffle) {
    pa = (mix64(seed ^ 0xa5a5a5a5ull) % (uint64_t)c->npos) | 1ull;
    while (gcd64(pa, (uint64_t)c->npos) != 1) pa += 2;
    pa %= (uint64_t)c->npos;
    if (pa == 0) pa = 1;
    pb = mix64(seed ^ 0x5a5a5a5aull) % (uint64_t)c->npos;
  }
  HIPCHK(hipMemsetAsync(c->bad, 0, 4, c->stream));
  HIPCHK(hipEventRecord(c->ev0, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    auto a = bpr_args<decltype(t)>(c, lr, bias_lambda, user_lambda, item_lambda, use_biases);
    a.num_neg = num_neg;
    a.seed = seed;
    a.perm_a = pa;
    a.perm_b = pb;
    c->bpr_waves = a.waves;
    c->bpr_atomic_user = a.atomic_user;
    HIPCHK(launch_bpr_epoch(a, c->kp, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev1, c->stream));
  int32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, c->bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  const double upd = (double)c->npos * num_neg;
  c->solve.add(ms, upd * 10.0 * c->k, upd * (6.0 * c->k * c->esz + 16 + 40));
  if (bad) return fail(kBadGradients, -4);
  return 0;
}

int qmfx_bpr_apply(qmfx_ctx* c, const int64_t* trip, int64_t n, double lr, double bias_lambda,
                   double user_lambda, double item_lambda, int use_biases) {
  if (set_dev(c)) return -2;
  if (int rc = ensure_side_factors(c, 0)) return rc;
  if (int rc = ensure_side_factors(c, 1)) return rc;
  if (int rc = ensure_bias(c)) return rc;
  if (!triplets_in_range(c, trip, n)) return fail("triplet index out of range");
  DevPtr<int64_t> d;
  HIPCHK(dev_alloc(d, (size_t)std::max<int64_t>(n, 1) * 24));
  HIPCHK(scopy(c, d, trip, (size_t)n * 24, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(c->bad, 0, 4, c->stream));
  const int rc = with_prec(c->prec, [&](auto t) {
    auto a = bpr_args<decltype(t)>(c, lr, bias_lambda, user_lambda, item_lambda, use_biases);
    HIPCHK(launch_bpr_apply(a, d, n, c->kp, c->stream));
    return 0;
  });
  if (rc) return rc;
  int32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, c->bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (bad) return fail(kBadGradients, -4);
  return 0;
}

int qmfx_bpr_eval(qmfx_ctx* c, int slot, const int64_t* trip, int64_t n, int use_biases,
                  double* loss_sum) {
  if (slot != 0 && slot != 1) return fail("slot must be 0 or 1");
  if (set_dev(c)) return -2;
  // (a changed shape releases the factors and the biases: zero again, as qmfx_bpr_apply's)
  if (int rc = ensure_side_factors(c, 0)) return rc;
  if (int rc = ensure_side_factors(c, 1)) return rc;
  if (int rc = ensure_bias(c)) return rc;
  if (c->trip_src[slot] != (const void*)trip || c->trip_n[slot] != n) {
    if (!triplets_in_range(c, trip, n)) return fail("triplet index out of range");
    HIPCHK(dev_alloc(c->trip[slot], (size_t)std::max<int64_t>(n, 1) * 24));
    HIPCHK(scopy(c, c->trip[slot], trip, (size_t)n * 24, hipMemcpyHostToDevice));
    c->trip_src[slot] = trip;
    c->trip_n[slot] = n;
  }
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    HIPCHK(launch_bpr_eval(c->s[0].F.as<const T>(), c->s[1].F.as<const T>(), c->bias.as<const T>(),
                           c->trip[slot], n, c->kp, use_biases, c->eval_partial, c->dsum,
                           c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(c->hsum, c->dsum, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *loss_sum = *c->hsum;
  return 0;
}

int qmfx_bpr_plan(qmfx_ctx* c, int* waves, int* atomic_user) {
  if (waves) *waves = c->bpr_waves;
  if (atomic_user) *atomic_user = c->bpr_atomic_user;
  return 0;
}

}  // extern "C"
