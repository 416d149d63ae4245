// Screened top-N recommendations (qmfx_recommend_screened): qmfx_recommend's lists, bit for bit,
// from an f32 MFMA scan of the catalogue that keeps what a certified bound cannot rule out
// (screen.hip) and an exact re-rank of the kept items (cand_select_kernel).  Stages:
//   0 sample    the exact top-N of S evenly spaced items per user (shared candidate list): the
//               score at rank N − 1 is the user's threshold L_u, a lower bound of the N-th best
//               score over the catalogue;
//   1 prepare   the requested rows gathered, both sides' norms, an fp64 context's f32 copies
//               (per call, never cached: any write to the factors would have to invalidate them);
//   2 screen    the scan; per user a counter and a list of at most `cap` items;
//   3 sort      the counters come to the host (the lists do not), which builds the candidate
//               offsets and work items; the kept lists become ascending through the radix sort
//               of data.hip on keys position << 32 | item (a sort of Σ list lengths keys, against
//               nusers × nitems bits for a bitmap compaction);
//   4 re-rank   qmfx_recommend_candidates' per-user form from the device-resident lists;
//   5 exact     users whose sample was short or whose counter ran past cap: gathered, answered
//               by the dense scan, scattered into place.
#include <cmath>

#include "ctx.h"

using namespace qmfx;

namespace {

// Catalogues below this go to the dense call when sample and cap are both auto: the screen's
// fixed stages (a dozen launches, a device-to-host round trip, the sort's allocation) do not
// pay off.  Not yet measured: a conservative guess below the 100K items where 4.3x was measured.
constexpr int64_t kScreenMinItems = 16384;

// auto sample: S = √(8 · topn · nitems), up to a multiple of 64, within topn..nitems (the sweep
// of DESIGN §3.12: the minimum of sample + screen + sort + re-rank at topn = 10 and 100)
int64_t auto_sample(int topn, int64_t ni) {
  int64_t s = (int64_t)std::ceil(std::sqrt(8.0 * topn * (double)ni));
  s = (s + 63) / 64 * 64;
  return std::max<int64_t>(std::min(s, ni), std::min<int64_t>(topn, ni));
}
// auto cap: four times the mean list length topn · nitems / S, plus 64
int64_t auto_cap(int topn, int64_t ni, int64_t S) { return 4 * topn * ni / S + 64; }

int dense(qmfx_ctx* c, int64_t nusers, const int64_t* users, int topn, int exclude, int use_biases,
          int64_t* items, double* scores, int32_t* counts) {
  c->scr.stats[1] = nusers;
  return recommend_dense(c, nusers, users, 0, nullptr, topn, exclude, use_biases, items, scores,
                         counts);
}

}  // namespace

extern "C" {

int qmfx_recommend_screened(qmfx_ctx* c, int64_t nusers, const int64_t* users, int topn,
                            int exclude, int use_biases, int64_t sample, int64_t cap,
                            int64_t* items, double* scores, int32_t* counts) {
  if (nusers == 0) return 0;
  if (int rc = rec_check(c, nusers, users, topn, exclude, use_biases)) return rc;
  const int64_t ni = c->s[1].n;
  if (sample != 0 && (sample < topn || sample > ni))
    return fail("sample must be 0 (auto) or in topn..nitems");
  if (cap != 0 && cap < topn) return fail("cap must be 0 (auto) or at least topn");
  Screen& x = c->scr;
  std::fill(x.stats, x.stats + 4, 0);
  std::fill(x.stage_ms, x.stage_ms + 6, 0.0);
  const bool all_auto = sample == 0 && cap == 0;
  if (ni == 0 || (all_auto && ni < kScreenMinItems))
    return dense(c, nusers, users, topn, exclude, use_biases, items, scores, counts);
  const int64_t S = sample ? sample : auto_sample(topn, ni);
  if (cap == 0) cap = auto_cap(topn, ni, S);
  // no list is longer than the catalogue; the packed lists are indexed with 31 bits
  cap = std::min(cap, ni);
  cap = std::min(cap, (((int64_t)1 << 31) - 1) / nusers);
  if (cap < 1 || screen_tiles(nusers, ni) > kScreenMaxTiles)
    return dense(c, nusers, users, topn, exclude, use_biases, items, scores, counts);
  if (set_dev(c)) return -2;

  TopN& s = c->rc;
  const size_t n = (size_t)nusers, kp = (size_t)c->kp;
  std::vector<int32_t> h_sample((size_t)S);
  for (int64_t j = 0; j < S; ++j) h_sample[(size_t)j] = (int32_t)(j * ni / S);  // S ≤ ni < 2^31
  if (int rc = topn_reserve_lists(c, nusers, (size_t)(cand_chunks(S) * eval_user_rows(nusers)),
                                  topn))
    return rc;
  if (int rc = reserve(s.cand, (size_t)S * 4)) return rc;
  if (int rc = reserve(x.ug, n * kp * c->esz)) return rc;
  if (c->prec == 64) {
    if (int rc = reserve(x.uf, n * kp * 4)) return rc;
    if (int rc = reserve(x.itf, (size_t)ni * kp * 4)) return rc;
  }
  if (int rc = reserve(x.unorm, n * 8)) return rc;
  if (int rc = reserve(x.inorm, (size_t)ni * 8)) return rc;
  if (int rc = reserve(x.thr, n * 8)) return rc;
  if (int rc = reserve(x.cnt, n * 4)) return rc;
  if (int rc = reserve(x.scnt, n * 4)) return rc;
  if (int rc = reserve(x.list, n * (size_t)cap * 4)) return rc;
  for (Event& e : x.ev)
    if (!e) HIPCHK(make_event(e));
  HIPCHK(scopy(c, s.users, users, n * 8, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, s.cand, h_sample.data(), (size_t)S * 4, hipMemcpyHostToDevice));

  // 0: thresholds from the sample
  HIPCHK(hipEventRecord(x.ev[0], c->stream));
  int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    CandArgs<T> a{};
    topn_args(c, a, nusers, ni, topn);
    rec_model(c, a, exclude, use_biases);
    a.cand = s.cand;
    a.ncand = S;
    HIPCHK(launch_recommend_candidates(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  HIPCHK(launch_screen_prep(s.scores, s.counts, nusers, topn, x.thr, x.cnt, x.scnt, c->stream));
  // 1: rows, norms, f32 copies
  HIPCHK(hipEventRecord(x.ev[1], c->stream));
  rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    T* ug = x.ug.as<T>();
    HIPCHK(launch_screen_gather(c->s[0].F.as<T>(), s.users, nusers, c->kp, ug, c->stream));
    HIPCHK(launch_factor_norms(ug, nusers, c->k, c->kp, x.unorm, c->stream));
    HIPCHK(launch_factor_norms(c->s[1].F.as<T>(), ni, c->k, c->kp, x.inorm, c->stream));
    return 0;
  });
  if (rc) return rc;
  const float *A = x.ug.as<float>(), *B = c->s[1].F.as<float>();
  if (c->prec == 64) {
    HIPCHK(launch_screen_f32(x.ug.as<double>(), (int64_t)(n * kp), x.uf, c->stream));
    HIPCHK(launch_screen_f32(c->s[1].F.as<double>(), ni * (int64_t)kp, x.itf, c->stream));
    A = x.uf;
    B = x.itf;
  }
  // 2: the scan
  HIPCHK(hipEventRecord(x.ev[2], c->stream));
  rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    ScreenArgs<T> a{};
    a.A = A;
    a.B = B;
    a.bias = use_biases ? c->bias.as<T>() : nullptr;
    a.nreq = nusers;
    a.nitems = ni;
    a.k = c->k;
    a.kp = c->kp;
    a.unorm = x.unorm;
    a.inorm = x.inorm;
    a.thr = x.thr;
    a.cnt = x.cnt;
    a.list = x.list;
    a.cap = cap;
    HIPCHK(launch_screen(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  // 3: counters to the host; offsets, work items and ascending lists
  HIPCHK(hipEventRecord(x.ev[3], c->stream));
  std::vector<int32_t> h_cnt(n), h_scnt(n), wuser;
  HIPCHK(scopy(c, h_cnt.data(), x.cnt, n * 4, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, h_scnt.data(), x.scnt, n * 4, hipMemcpyDeviceToHost));
  std::vector<int64_t> cptr(n + 1, 0), woff(n + 1, 0), xpos, xusers;
  int64_t longest = 0;
  for (size_t t = 0; t < n; ++t) {
    const bool exact = h_scnt[t] < topn || h_cnt[t] > cap;
    const int64_t len = exact ? 0 : h_cnt[t];
    if (exact) {
      xpos.push_back((int64_t)t);
      xusers.push_back(users[t]);
    }
    longest = std::max(longest, len);
    cptr[t + 1] = cptr[t] + len;
    woff[t + 1] = woff[t] + cand_chunks(len);
  }
  const int64_t total = cptr[n], nx = (int64_t)xpos.size();
  wuser.resize((size_t)woff[n]);
  for (size_t t = 0; t < n; ++t)
    std::fill(wuser.begin() + woff[t], wuser.begin() + woff[t + 1], (int32_t)t);
  const size_t np = (n + 1) * 8;
  if (int r = reserve(s.cptr, np)) return r;
  if (int r = reserve(s.woff, np)) return r;
  if (int r = reserve(s.wuser, std::max<size_t>(wuser.size() * 4, 16))) return r;
  if (int r = reserve(s.cand, std::max<size_t>((size_t)total * 4, 16))) return r;
  if (int r = reserve(x.keys, std::max<size_t>((size_t)total * 8, 16))) return r;
  if (int r = reserve(x.keys2, std::max<size_t>((size_t)total * 8, 16))) return r;
  // the partial lists of the re-rank (one per work item) and of the exact scan; the request's
  // rows and outputs keep their buffers
  const size_t xout = (size_t)nx * (size_t)topn;
  const size_t xlists = nx > 0 ? (size_t)(eval_chunks(nx, ni) * eval_user_rows(nx)) : 0;
  if (int r = topn_reserve_lists(c, nusers, std::max((size_t)woff[n], xlists), topn)) return r;
  if (nx > 0) {
    if (int r = reserve(x.xusers, (size_t)nx * 8)) return r;
    if (int r = reserve(x.xitems, xout * 8)) return r;
    if (int r = reserve(x.xscores, xout * 8)) return r;
    if (int r = reserve(x.xcounts, (size_t)nx * 4)) return r;
    HIPCHK(scopy(c, x.xusers, xusers.data(), (size_t)nx * 8, hipMemcpyHostToDevice));
  }
  HIPCHK(scopy(c, s.cptr, cptr.data(), np, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, s.woff, woff.data(), np, hipMemcpyHostToDevice));
  HIPCHK(scopy(c, s.wuser, wuser.data(), wuser.size() * 4, hipMemcpyHostToDevice));
  if (total > 0) {
    int ubits = 1;
    while (((int64_t)1 << ubits) < nusers) ++ubits;
    HIPCHK(launch_screen_keys(x.list, s.cptr, nusers, cap, x.keys, c->stream));
    HIPCHK(sort_keys(x.keys, x.keys2, total, 32 + ubits, c->stream));
    HIPCHK(launch_screen_unpack(x.keys, total, s.cand, c->stream));
  }
  // 4: the exact re-rank of everyone's kept items (an exact-scan user's list is empty here)
  HIPCHK(hipEventRecord(x.ev[4], c->stream));
  rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    CandArgs<T> a{};
    topn_args(c, a, nusers, ni, topn);
    rec_model(c, a, exclude, use_biases);
    a.cand = s.cand;
    a.cptr = s.cptr;
    a.woff = s.woff;
    a.wuser = s.wuser;
    a.h_woff = woff.data();
    HIPCHK(launch_recommend_candidates(a, c->stream));
    return 0;
  });
  if (rc) return rc;
  // 5: the exact scan of the others, into buffers of its own
  HIPCHK(hipEventRecord(x.ev[5], c->stream));
  if (nx > 0) {
    rc = with_prec(c->prec, [&](auto t) {
      using T = decltype(t);
      RecArgs<T> a{};
      topn_args(c, a, nx, ni, topn);
      rec_model(c, a, exclude, use_biases);
      a.users = x.xusers;
      a.items = x.xitems;
      a.scores = x.xscores;
      a.counts = x.xcounts;
      HIPCHK(launch_recommend(a, c->stream));
      return 0;
    });
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(x.ev[6], c->stream));

  if (int r = topn_copy_out(c, nusers, topn, items, scores, counts)) return r;
  if (nx > 0) {
    std::vector<int64_t> xi(xout);
    std::vector<double> xs(xout);
    std::vector<int32_t> xc((size_t)nx);
    HIPCHK(scopy(c, xi.data(), x.xitems, xout * 8, hipMemcpyDeviceToHost));
    HIPCHK(scopy(c, xs.data(), x.xscores, xout * 8, hipMemcpyDeviceToHost));
    HIPCHK(scopy(c, xc.data(), x.xcounts, (size_t)nx * 4, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < (size_t)nx; ++j) {
      const size_t t = (size_t)xpos[j];
      std::copy_n(xi.begin() + j * topn, topn, items + t * topn);
      std::copy_n(xs.begin() + j * topn, topn, scores + t * topn);
      counts[t] = xc[j];
    }
  }
  x.stats[0] = nusers - nx;
  x.stats[1] = nx;
  x.stats[2] = total;
  x.stats[3] = longest;
  // the stages' time (stage 3 holds the counters' round trip), for qmfx_solve_kernel_stats:
  // 2k flop per (user, item scanned), as the dense call accounts itself
  double ms_all = 0;
  for (int i = 0; i < 6; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, x.ev[i], x.ev[i + 1]));
    x.stage_ms[i] = ms;
    ms_all += ms;
  }
  c->solve.add(ms_all, topn_flops(c, nusers, ni), topn_bytes(c, nusers, ni));
  return 0;
}

int qmfx_recommend_screen_stats(qmfx_ctx* c, int64_t out[4]) {
  std::copy(c->scr.stats, c->scr.stats + 4, out);
  return 0;
}

int qmfx_recommend_screen_stage_ms(qmfx_ctx* c, double out[6]) {
  std::copy(c->scr.stage_ms, c->scr.stage_ms + 6, out);
  return 0;
}

}  // extern "C"
