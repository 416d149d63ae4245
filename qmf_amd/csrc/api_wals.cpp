// One WALS half-epoch in phases, and the per-row diagnostics.  qmfx_wals_half runs the
// phases in order on one context; qmfx_wals_half_multi interleaves them over several contexts
// (one process driving several GPUs) so that piece j's all-gather of every context is one
// RCCL group while piece j+1 computes.
#include <cstdio>

#include "rows.h"

using namespace qmfx;

namespace {

ncclDataType_t nccl_type(int prec) { return prec == 32 ? ncclFloat32 : ncclFloat64; }

// G = YᵀY, the whitening and G + λI images, status resets (no collectives)
template <typename T>
int half_begin_t(qmfx_ctx* c, int side, double alpha, double lambda) {
  SideBuf& L = c->s[side];
  SideBuf& R = c->s[1 - side];
  if (!L.rowptr) return fail("no interactions uploaded for the solved side");
  if (!L.buckets_valid) return fail("row buckets not built");
  if (c->comm_aborted)
    return fail("the RCCL clique was aborted after a failed collective; recreate the contexts");
  if (set_dev(c)) return -2;
  if (int rc = ensure_side_factors(c, side)) return rc;
  if (int rc = ensure_side_factors(c, 1 - side)) return rc;
  if (int rc = ensure_rowloss(c, L.n)) return rc;
  const int64_t nW = L.wb[kMaxNTN];             // whitened rows (all buckets)
  const bool use_w = nW > 0 && lambda > 0.0;    // M = YᵀY + λI is SPD only for λ > 0
  c->hs = qmfx_ctx::HalfStateT{side, alpha, lambda, use_w, 0, std::getenv("QMFX_TRACE")};
  HIPCHK(hipEventRecord(c->evh[0], c->stream));
  if (int rc = fixed_side_prologue<T>(c, R, lambda, use_w)) return rc;
  HIPCHK(hipMemsetAsync(c->status, 0, (size_t)std::max<int64_t>(L.n, 1) * sizeof(int32_t), c->stream));
  HIPCHK(hipMemsetAsync(c->fb_cnt, 0, 2 * sizeof(unsigned long long), c->stream));
  const char* trace_path = c->hs.trace_path;
  if (trace_path && c->trace_cap < L.n_ord) {
    HIPCHK(dev_alloc(c->trace, (size_t)L.n_ord * 64));
    c->trace_cap = L.n_ord;
  }
  if (trace_path) HIPCHK(hipMemsetAsync(c->trace, 0, (size_t)L.n_ord * 64, c->stream));
  return 0;
}

int half_begin(qmfx_ctx* c, int side, double alpha, double lambda) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  return with_prec(c->prec, [&](auto t) { return half_begin_t<decltype(t)>(c, side, alpha, lambda); });
}

// the row solves of piece j (direct, heavy, whitened, pivoted re-solve before the all-gather);
// records evp[j][0..2]: start, direct done, whitened done
template <typename T>
int half_piece_t(qmfx_ctx* c, int j) {
  if (set_dev(c)) return -2;
  const qmfx_ctx::HalfStateT& hs = c->hs;
  SideBuf& L = c->s[hs.side];
  const Piece& pc = L.pieces[j];
  c->hs.nD += pc.n_ord - (hs.use_w ? pc.wb[kMaxNTN] : 0);
  HIPCHK(hipEventRecord(c->evp[j][0], c->stream));
  if (int rc = solve_rows<T>(c, side_rows<T>(c, L), c->s[1 - hs.side], pc.ord, pc.n_ord, pc.wb,
                             hs.alpha, hs.lambda, hs.use_w, SplitK{&L, pc.nh, pc.h0, pc.s0, pc.ns},
                             hs.trace_path ? c->trace.get() : nullptr, c->evp[j][1]))
    return rc;
  HIPCHK(hipEventRecord(c->evp[j][2], c->stream));
  return 0;
}

int half_piece(qmfx_ctx* c, int j) {
  return with_prec(c->prec, [&](auto t) { return half_piece_t<decltype(t)>(c, j); });
}

// piece j of this rank → every rank (one ncclGroup; nests inside a caller's group)
int half_comm_piece(qmfx_ctx* c, int j) {
  if (set_dev(c)) return -2;
  // fault injection for the clique's failure path (tests): QMFX_FAULT_COMM_RANK=<rank>
  if (c->comm && c->fault_comm_rank == c->rank && c->comm_pieces_done++ >= c->fault_comm_after)
    return fail("injected collective failure", -3);
  SideBuf& L = c->s[c->hs.side];
  const int P = (int)L.pieces.size();
  if (c->comm) {
    // piece j of every rank → every rank (an all-gather-v of contiguous row ranges), on
    // the collective stream while the next piece is solved
    HIPCHK(hipStreamWaitEvent(c->comm_stream, c->evp[j][2], 0));
    HIPCHK(hipEventRecord(c->evx[j][0], c->comm_stream));
    NCCLCHK(ncclGroupStart());
    for (int r = 0; r < c->world; ++r) {
      const int64_t b = L.pbounds[(size_t)r * (P + 1) + j], e = L.pbounds[(size_t)r * (P + 1) + j + 1];
      if (e <= b) continue;
      char* base = L.F.as<char>() + (size_t)b * c->kp * c->esz;
      NCCLCHK(ncclBroadcast(base, base, (size_t)(e - b) * c->kp, nccl_type(c->prec), r, c->comm,
                            c->comm_stream));
    }
    NCCLCHK(ncclGroupEnd());
    HIPCHK(hipEventRecord(c->evx[j][1], c->comm_stream));
  }
  return 0;
}

// trace dump (diagnostics), the loss sum and the status block
int half_tail(qmfx_ctx* c) {
  if (set_dev(c)) return -2;
  const int side = c->hs.side;
  const char* trace_path = c->hs.trace_path;
  SideBuf& L = c->s[side];
  if (trace_path) {
    std::vector<uint64_t> h((size_t)L.n_ord * 8);
    HIPCHK(scopy(c, h.data(), c->trace, h.size() * 8, hipMemcpyDeviceToHost));
    const std::string fn = std::string(trace_path) + "_side" + std::to_string(side) + ".bin";
    if (FILE* f = std::fopen(fn.c_str(), "wb")) {
      std::fwrite(h.data(), 8, h.size(), f);
      std::fclose(f);
    }
  }
  HIPCHK(launch_sum_f64(c->rowloss + L.rbeg, L.rend - L.rbeg, c->dsum, c->stream));
  // loss, re-solve counts and the factorization flag in one status block
  HIPCHK(launch_half_status(c->dsum, c->fb_cnt, c->hs.use_w ? c->chol_status.get() : nullptr,
                            c->dsum + kHalfStatus, c->stream));
  return 0;
}

int half_comm_status(qmfx_ctx* c) {
  if (set_dev(c)) return -2;
  if (c->comm) {
    // the whole status block is summed over the ranks, so every rank sees the same
    // singular-row count and fails (-6) in the same half instead of leaving the others in
    // the next half's collectives
    HIPCHK(hipEventRecord(c->ev_sum, c->stream));
    HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_sum, 0));
    NCCLCHK(ncclAllReduce(c->dsum + kHalfStatus, c->dsum + kHalfStatus, 4, ncclFloat64, ncclSum,
                          c->comm, c->comm_stream));
    HIPCHK(hipEventRecord(c->ev_comm, c->comm_stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_comm, 0));
  }
  return 0;
}

int half_end(qmfx_ctx* c, double* loss_sum) {
  if (set_dev(c)) return -2;
  SideBuf& L = c->s[c->hs.side];
  const int P = (int)L.pieces.size();
  HIPCHK(hipEventRecord(c->evh[2], c->stream));
  if (int rc = read_half_status(c)) return rc;
  c->fb_rows = (int64_t)c->hsum[1];
  if (int rc = half_status_failure(c)) return rc;
  // timing and algorithmic work per kernel class (SURVEY.md §8(d) accounting)
  float ms_d = 0.f, ms_w = 0.f, ms_h = 0.f;
  for (int j = 0; j < P; ++j) {
    float t0 = 0.f, t1 = 0.f;
    HIPCHK(hipEventElapsedTime(&t0, c->evp[j][0], c->evp[j][1]));
    HIPCHK(hipEventElapsedTime(&t1, c->evp[j][1], c->evp[j][2]));
    ms_d += t0;
    ms_w += t1;
  }
  HIPCHK(hipEventElapsedTime(&ms_h, c->evh[0], c->evh[2]));
  const double k = c->k, s = (double)c->esz;
  const int sd = c->hs.side;
  if (c->comm) {
    // the exchange on the collective stream (the status all-reduce behind the last piece's
    // broadcasts has completed: the host synchronised on it above)
    float xb = 0.f, tail = 0.f;
    for (int j = 0; j < P; ++j) {
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, c->evx[j][0], c->evx[j][1]));
      xb += t;
    }
    HIPCHK(hipEventElapsedTime(&tail, c->evp[P - 1][2], c->evx[P - 1][1]));
    c->xch_ms[sd] += xb;
    c->xch_tail_ms[sd] += tail;
    c->xch_solve_ms[sd] += ms_d + ms_w;
    c->xch_halves[sd] += 1;
  }
  auto acc = [&](int cls, double ms, double fl, double by) {
    c->cls[cls].add(ms, fl, by);
    c->side[sd][cls].add(ms, fl, by);
  };
  const bool use_w = c->hs.use_w;
  const int64_t nD = c->hs.nD, nW = L.wb[kMaxNTN];
  const double nzd = use_w ? L.nnz_d : L.nnz_d + L.nnz_w, nd = (double)nD;
  const double nzw = use_w ? L.nnz_w : 0.0, nw = use_w ? (double)nW : 0.0;
  double fl_d = 0, by_d = 0, fl_w = 0, by_w = 0;
  if (nD > 0) {
    fl_d = direct_flops(c, nzd, nd);
    by_d = direct_bytes(c, nzd, nd);
    acc(0, ms_d, fl_d, by_d);
  }
  if (nW > 0 && use_w) {
    // whitened-row flops precomputed per side in build_buckets; bytes as SURVEY.md §8(d):
    // signals, gathered rows, X write, rowptr (the x' round trip of the unwhitening pass,
    // 2·k·s per row, is reported beside them by bench.py as extra_bytes)
    fl_w = L.flops_w;
    by_w = nzw * (4 + s) + nzw * k * s + nw * k * s + (nw + 1) * 8;
    acc(1, ms_w, fl_w, by_w);
  }
  acc(2, ms_h, fl_d + fl_w, by_d + by_w);
  c->solve.add(ms_d + ms_w, fl_d + fl_w, by_d + by_w);
  c->last_side = c->hs.side;
  if (loss_sum) *loss_sum = *c->hsum;
  return 0;
}

}  // namespace

extern "C" {

int qmfx_wals_half(qmfx_ctx* c, int side, double alpha, double lambda, double* loss_sum) {
  if (int rc = half_begin(c, side, alpha, lambda)) return rc;
  const int P = (int)c->s[side].pieces.size();
  for (int j = 0; j < P; ++j) {
    if (int rc = half_piece(c, j)) return rc;
    if (int rc = half_comm_piece(c, j)) return rc;
  }
  if (int rc = half_tail(c)) return rc;
  if (c->comm) {
    NCCLCHK(ncclGroupStart());
    const int rc = half_comm_status(c);
    NCCLCHK(ncclGroupEnd());
    if (rc) return rc;
  }
  return half_end(c, loss_sum);
}

int qmfx_wals_half_multi(qmfx_ctx* const* ctxs, int n, int side, double alpha, double lambda,
                         double* loss_sum) {
  if (n < 1 || !ctxs) return fail("no contexts");
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return fail("null context");
    if (n > 1 && (!ctxs[i]->comm || ctxs[i]->world != n || ctxs[i]->rank != i))
      return fail("contexts must come from one qmfx_dist_init_all, in rank order");
  }
  for (int i = 0; i < n; ++i)
    if (int rc = half_begin(ctxs[i], side, alpha, lambda)) return rc;
  const int P = (int)ctxs[0]->s[side].pieces.size();
  for (int i = 1; i < n; ++i)
    if ((int)ctxs[i]->s[side].pieces.size() != P) return fail("contexts disagree on the pieces");
  // A context that fails after others have posted their part of a group would leave those
  // collectives waiting for peers that never join, and the next sync would hang: abort every
  // communicator of the clique instead (outstanding collectives are cancelled), so the call
  // returns the error and later calls on these contexts fail loudly.
  auto abort_clique = [&](int rc) {
    for (int i = 0; i < n; ++i) {
      if (ctxs[i]->comm) {
        (void)ncclCommAbort(ctxs[i]->comm);
        ctxs[i]->comm = nullptr;
        ctxs[i]->comm_aborted = true;
      }
    }
    return rc;
  };
  for (int j = 0; j < P; ++j) {
    for (int i = 0; i < n; ++i)
      if (int rc = half_piece(ctxs[i], j)) return abort_clique(rc);
    // one thread drives every communicator: all ranks' broadcasts of piece j in one group
    NCCLCHK(ncclGroupStart());
    int rc = 0;
    for (int i = 0; i < n && rc == 0; ++i) rc = half_comm_piece(ctxs[i], j);
    const ncclResult_t ge = ncclGroupEnd();
    if (rc) return abort_clique(rc);
    if (ge != ncclSuccess) return abort_clique(fail(std::string("RCCL: ") + ncclGetErrorString(ge), -4));
  }
  for (int i = 0; i < n; ++i)
    if (int rc = half_tail(ctxs[i])) return abort_clique(rc);
  {
    NCCLCHK(ncclGroupStart());
    int rc = 0;
    for (int i = 0; i < n && rc == 0; ++i)
      if (ctxs[i]->comm) rc = half_comm_status(ctxs[i]);
    const ncclResult_t ge = ncclGroupEnd();
    if (rc) return abort_clique(rc);
    if (ge != ncclSuccess) return abort_clique(fail(std::string("RCCL: ") + ncclGetErrorString(ge), -4));
  }
  double first = 0.0;
  for (int i = 0; i < n; ++i) {
    double l = 0.0;
    if (int rc = half_end(ctxs[i], &l)) return rc;
    if (i == 0) first = l;
  }
  if (loss_sum) *loss_sum = first;
  return 0;
}

int qmfx_row_classes(qmfx_ctx* c, int side, int64_t* counts) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  const SideBuf& sb = c->s[side];
  if (!sb.buckets_valid) return fail("row buckets not built");
  for (int i = 0; i < kMaxNTN + 3; ++i) counts[i] = 0;
  for (const auto& pc : sb.pieces) {
    for (int b = 0; b < kMaxNTN; ++b) counts[b] += pc.wb[b + 1] - pc.wb[b];
    counts[kMaxNTN] += pc.n_ord - pc.wb[kMaxNTN] - pc.nh;
    counts[kMaxNTN + 1] += pc.nh;
    counts[kMaxNTN + 2] += pc.ns;
  }
  return 0;
}

int qmfx_wals_row_losses(qmfx_ctx* c, double* out) {
  const SideBuf& L = c->s[c->last_side];
  if (!c->rowloss || c->rowloss_cap < L.n) return fail("no half solved yet");
  if (set_dev(c)) return -2;
  HIPCHK(scopy(c, out, c->rowloss, (size_t)L.n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int qmfx_wals_failed_rows(qmfx_ctx* c, int64_t* rows, int64_t cap, int64_t* count) {
  SideBuf& L = c->s[c->last_side];
  if (!c->status || c->rowloss_cap < L.n) return fail("no half solved yet");
  if (set_dev(c)) return -2;
  std::vector<int32_t> st((size_t)std::max<int64_t>(L.n, 1));
  HIPCHK(scopy(c, st.data(), c->status, st.size() * 4, hipMemcpyDeviceToHost));
  int64_t cnt = 0;
  for (int64_t r = 0; r < L.n; ++r)
    if (st[r]) {
      if (cnt < cap && rows) rows[cnt] = r;
      ++cnt;
    }
  *count = cnt;
  return 0;
}

int qmfx_wals_row_system(qmfx_ctx* c, int side, int64_t row, double alpha, double lambda,
                         double* A, double* b, double* csum) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  SideBuf& L = c->s[side];
  SideBuf& R = c->s[1 - side];
  if (row < 0 || row >= L.n) return fail("row out of range");
  if (!L.rowptr) return fail("no interactions uploaded for this side");
  if (L.sharded && (row < L.rbeg || row >= L.rend)) return fail("row not held by this rank");
  if (set_dev(c)) return -2;
  if (int rc = ensure_side_factors(c, 1 - side)) return rc;
  const size_t k = c->k, nout = k * k + k + 1;
  DevPtr<double> d;
  HIPCHK(dev_alloc(d, nout * sizeof(double)));
  const int64_t beg = L.h_rowptr[row], end = L.h_rowptr[row + 1];
  std::vector<double> h(nout);
  const int rc = with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    // YᵀY of this side's fixed side (the last half may have solved the other side)
    HIPCHK(launch_gram_t<T>(c, R));
    hipError_t e = launch_wals_system(
        fallback_args<T>(c, side_rows<T>(c, L), R, 0, 0, alpha, lambda), beg, end, d, c->stream);
    if (e == hipSuccess) e = scopy(c, h.data(), d, nout * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(std::string("qmfx_wals_row_system: ") + hipGetErrorString(e), -2);
    return 0;
  });
  if (rc) return rc;
  std::copy(h.begin(), h.begin() + k * k, A);
  std::copy(h.begin() + k * k, h.begin() + k * k + k, b);
  if (csum) *csum = h[k * k + k];
  return 0;
}

int qmfx_wals_set_row(qmfx_ctx* c, int side, int64_t row, const double* x) {
  SideBuf& L = c->s[side];
  if (row < 0 || row >= L.n) return fail("row out of range");
  if (set_dev(c)) return -2;
  const int kp = c->kp, k = c->k;
  return with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    std::vector<T> h(kp, T(0));
    for (int i = 0; i < k; ++i) h[i] = (T)x[i];
    HIPCHK(scopy(c, L.F.as<T>() + (size_t)row * kp, h.data(), kp * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  });
}

}  // extern "C"
