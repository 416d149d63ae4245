// qmfx_wals_half_cg: one WALS half whose rows take a few warm-started conjugate-gradient steps
// (wals_cg.hip) instead of the exact solve.  Rows of the split-K heavy class are solved exactly
// by the launch sequence of the exact half (rows.h).  One device only.
#include "rows.h"

using namespace qmfx;

namespace {

template <typename T>
int half_cg_t(qmfx_ctx* c, int side, double alpha, double lambda, int steps, double* loss_sum) {
  SideBuf& L = c->s[side];
  SideBuf& R = c->s[1 - side];
  if (set_dev(c)) return -2;
  // a side never set starts from x₀ = 0; a side that holds values keeps them (the warm start)
  if (int rc = ensure_side_factors(c, side)) return rc;
  if (int rc = ensure_rowloss(c, L.n)) return rc;
  HIPCHK(hipEventRecord(c->evh[0], c->stream));
  // G = YᵀY; the heavy rows' kernels also read G + λI's tile image
  if (L.nheavy > 0) {
    if (int rc = fixed_side_prologue<T>(c, R, lambda, false)) return rc;
  } else {
    HIPCHK(launch_gram_t<T>(c, R));
  }
  HIPCHK(hipMemsetAsync(c->status, 0, (size_t)std::max<int64_t>(L.n, 1) * sizeof(int32_t), c->stream));
  HIPCHK(hipMemsetAsync(c->fb_cnt, 0, 2 * sizeof(unsigned long long), c->stream));
  const Rows<T> v = side_rows<T>(c, L);
  CgArgs<T> a{v.col, v.val, R.F.as<T>(), c->G.as<T>(), v.X, v.rowloss, v.status, v.desc,
              0,     0,     (T)alpha,    (T)lambda,    steps};
  const int64_t no_buckets[kMaxNTN + 1] = {};
  for (const Piece& pc : L.pieces) {
    // the piece's slots: [whitened classes | heavy rows | other direct rows]
    const int64_t h = pc.ord + pc.wb[kMaxNTN];
    if (pc.nh > 0)
      if (int rc = solve_rows<T>(c, v, R, h, pc.nh, no_buckets, alpha, lambda, false,
                                 SplitK{&L, pc.nh, pc.h0, pc.s0, pc.ns}))
        return rc;
    const int64_t range[2][2] = {{pc.ord, h}, {h + pc.nh, pc.ord + pc.n_ord}};
    for (const auto& r : range) {
      a.slot_begin = r[0];
      a.nslots = r[1] - r[0];
      HIPCHK(launch_wals_cg(a, c->nt, c->stream));
    }
  }
  HIPCHK(launch_sum_f64(c->rowloss + L.rbeg, L.rend - L.rbeg, c->dsum, c->stream));
  HIPCHK(launch_half_status(c->dsum, c->fb_cnt, nullptr, c->dsum + kHalfStatus, c->stream));
  HIPCHK(hipEventRecord(c->evh[2], c->stream));
  if (int rc = read_half_status(c)) return rc;
  c->fb_rows = (int64_t)c->hsum[1];
  c->last_side = side;
  if (int rc = half_status_failure(c)) return rc;
  // work: (steps + 1) operator applications of 2k² + 4nk per CG row, the exact formula for
  // the heavy rows
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->evh[0], c->evh[2]));
  double nz_h = 0, n_h = 0;
  if (L.nheavy > 0) {
    const int mx = max_whitened_ntn(c);
    for (int64_t r = L.rbeg; r < L.rend; ++r) {
      const int64_t n = L.h_rowptr[r + 1] - L.h_rowptr[r];
      if (n > c->heavy_min && (n + 15) / 16 > mx) nz_h += (double)n, n_h += 1;
    }
  }
  const double k = c->k, s = (double)c->esz, ap = steps + 1.0;
  const double nz = L.nnz_w + L.nnz_d - nz_h, nr = (double)L.n_ord - n_h;
  const double fl = ap * (2 * k * k * nr + 4 * k * nz) + direct_flops(c, nz_h, n_h);
  const double by = ap * nz * (4 + s + k * s) + 2 * nr * k * s + direct_bytes(c, nz_h, n_h);
  c->solve.add(ms, fl, by);
  c->cls[2].add(ms, fl, by);
  c->side[side][2].add(ms, fl, by);
  if (loss_sum) *loss_sum = *c->hsum;
  return 0;
}

}  // namespace

extern "C" int qmfx_wals_half_cg(qmfx_ctx* c, int side, double alpha, double lambda, int steps,
                                 double* loss_sum) {
  if (!c) return fail("null context");
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  if (steps < 1) return fail("steps must be at least 1");
  if (c->comm || c->world > 1 || c->comm_aborted)
    return fail("qmfx_wals_half_cg runs on one device: this context is sharded (qmfx_dist_init)");
  if (c->k > 16 * kCgMaxNT) return fail("qmfx_wals_half_cg supports at most 256 factors");
  const SideBuf& L = c->s[side];
  if (!L.rowptr) return fail("no interactions uploaded for the solved side");
  if (!L.buckets_valid) return fail("row buckets not built");
  if (!c->s[1 - side].F) return fail("the fixed side has no factors (qmfx_set_factors / qmfx_fill_uniform)");
  return with_prec(c->prec, [&](auto t) {
    return half_cg_t<decltype(t)>(c, side, alpha, lambda, steps, loss_sum);
  });
}
