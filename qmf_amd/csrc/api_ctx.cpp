// Host side of the qmfx C ABI (include/qmfx.h): the context's lifecycle, shape and factors,
// the kernel statistics and the MFMA self-test.  The other api_*.cpp units hold the signals
// and row buckets, the WALS half-epoch, BPR, test-set evaluation and the RCCL data path.
#include <cstring>
#include <memory>

#include "ctx.h"

using namespace qmfx;

thread_local std::string qmfx::g_err;

extern "C" {

const char* qmfx_last_error(void) { return g_err.c_str(); }
int qmfx_version(void) { return 1; }

int qmfx_device_count(int* count) {
  HIPCHK(hipGetDeviceCount(count));
  return 0;
}

int qmfx_create(qmfx_ctx** out, int device, int precision, int nfactors) {
  if (!out) return fail("out is null");
  if (precision != 32 && precision != 64) return fail("precision must be 32 or 64");
  if (nfactors <= 0) return fail("nfactors must be positive");
  const int nt = (nfactors + 15) / 16;
  if (nt > 16) return fail("nfactors > 256 not supported yet");
  // a failed create releases whatever it had made
  std::unique_ptr<qmfx_ctx> c(new qmfx_ctx());
  if (nt > 8) c->gpart_blocks = 256;  // YᵀY partials: NTT·256 doubles per block
  c->device = device;
  c->prec = precision;
  c->k = nfactors;
  c->nt = nt;
  c->kp = 16 * nt;
  c->esz = precision == 32 ? 4 : 8;
  if (const char* nw = std::getenv("QMFX_NO_WHITEN")) c->whitened_enabled = std::atoi(nw) == 0;
  if (const char* w = std::getenv("QMFX_WB_K64_NTN")) c->wb_k64_ntn = std::min(std::max(std::atoi(w), 1), 4);
  if (const char* f = std::getenv("QMFX_FAULT_COMM_RANK")) {
    c->fault_comm_rank = std::atoi(f);
    if (const char* a = std::strchr(f, ':')) c->fault_comm_after = std::atoll(a + 1);
  }
  if (const char* hm = std::getenv("QMFX_HEAVY_MIN")) c->heavy_min = std::max<int64_t>(std::atoll(hm), 0);
  if (const char* sl = std::getenv("QMFX_SEG_LEN"))
    c->seg_len = std::min<int64_t>(std::max<int64_t>(std::atoll(sl), 64), INT32_MAX);
  if (const char* np = std::getenv("QMFX_PIECES"))
    c->npieces = std::min(std::max(std::atoi(np), 1), QMFX_MAX_PIECES);
  const size_t ntt = (size_t)nt * (nt + 1) / 2, kp = c->kp;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess)
    e = hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess) e = make_stream(c->stream);
  if (e == hipSuccess) e = dev_alloc(c->G, kp * kp * c->esz);
  if (e == hipSuccess)
    e = dev_alloc(c->gpart, (size_t)c->gpart_blocks * ntt * 256 * sizeof(double));
  // sum + partials (launch_sum_f64: 1 + kSumBlocks), then the half status block
  if (e == hipSuccess) e = dev_alloc(c->dsum, (kHalfStatus + 4) * sizeof(double));
  if (e == hipSuccess) e = pinned_alloc(c->hsum, 4 * sizeof(double));
  if (e == hipSuccess) e = dev_alloc(c->bad, sizeof(int32_t));
  if (e == hipSuccess) e = dev_alloc(c->eval_partial, 1024 * sizeof(double));
  if (e == hipSuccess) e = make_event(c->ev0);
  if (e == hipSuccess) e = make_event(c->ev1);
  for (int i = 0; i < 4 && e == hipSuccess; ++i) e = make_event(c->evh[i]);
  for (int i = 0; i < QMFX_MAX_PIECES && e == hipSuccess; ++i)
    for (int j = 0; j < 3 && e == hipSuccess; ++j) e = make_event(c->evp[i][j]);
  for (int i = 0; i < QMFX_MAX_PIECES && e == hipSuccess; ++i)
    for (int j = 0; j < 2 && e == hipSuccess; ++j) e = make_event(c->evx[i][j]);
  if (e == hipSuccess) e = make_event(c->ev_sum, hipEventDisableTiming);
  if (e == hipSuccess) e = make_event(c->ev_comm, hipEventDisableTiming);
  if (e == hipSuccess) e = dev_alloc(c->Linv, kp * kp * c->esz);
  if (e == hipSuccess) e = dev_alloc(c->Gimg, ntt * 256 * c->esz);
  if (e == hipSuccess) e = dev_alloc(c->chol_status, sizeof(int32_t));
  if (e == hipSuccess && kp > 128) e = dev_alloc(c->chol_scratch, kp * (kp + 1) * sizeof(double));
  if (e == hipSuccess)
    e = dev_alloc(c->fb_scratch, (size_t)FB_MAX_GRID * (kp + 3) * kp * sizeof(double));
  if (e == hipSuccess) e = dev_alloc(c->fb_cnt, 2 * sizeof(unsigned long long));
  if (e != hipSuccess) return fail(std::string("qmfx_create: ") + hipGetErrorString(e), -2);
  *out = c.release();
  return 0;
}

int qmfx_destroy(qmfx_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
  if (c->comm) ncclCommDestroy(c->comm);
  delete c;  // events and buffers, then the streams (the order of qmfx_ctx's members)
  return 0;
}

int qmfx_sync(qmfx_ctx* c) {
  if (set_dev(c)) return -2;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int qmfx_set_shape(qmfx_ctx* c, int64_t nusers, int64_t nitems) {
  if (nusers <= 0 || nitems <= 0) return fail("empty shape: nusers and nitems must be > 0");
  if (nitems > 0x7fffffffll || nusers > 0x7fffffffll) return fail("more than 2^31 rows");
  if (set_dev(c)) return -2;
  const bool users_changed = c->s[0].n != nusers, items_changed = c->s[1].n != nitems;
  for (int side = 0; side < 2; ++side) {
    const int64_t n = side == 0 ? nusers : nitems;
    c->s[side].h_ids.clear();
    if (c->s[side].n != n) {
      c->s[side].F.reset();
      drop_csr(c->s[side]);
      c->s[side].h_rowptr.clear();
      c->s[side].buckets_valid = false;
      c->s[side].n = n;
    }
  }
  // What was sized or indexed by the old row counts goes with them; a call that needs it
  // fails until it is set again (scratch behind a capacity check, such as rowloss, Z and
  // every Scratch buffer, regrows on demand and stays).
  if (users_changed || items_changed) {
    drop_eval_labels(c);
    drop_bpr_positives(c);
  }
  if (items_changed) c->bias.reset();
  return 0;
}

int qmfx_get_shape(qmfx_ctx* c, int64_t* nusers, int64_t* nitems, int64_t* nnz) {
  if (nusers) *nusers = c->s[0].n;
  if (nitems) *nitems = c->s[1].n;
  if (nnz) *nnz = c->nnz;
  return 0;
}

int qmfx_set_factors(qmfx_ctx* c, int side, const double* f) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  if (set_dev(c)) return -2;
  if (int rc = ensure_side_factors(c, side)) return rc;
  SideBuf& sb = c->s[side];
  const size_t n = (size_t)sb.n, kp = c->kp, k = c->k;
  return with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    std::vector<T> h(n * kp, T(0));
    for (size_t r = 0; r < n; ++r)
      for (size_t j = 0; j < k; ++j) h[r * kp + j] = (T)f[r * k + j];
    HIPCHK(scopy(c, sb.F, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  });
}

int qmfx_get_factors(qmfx_ctx* c, int side, double* f) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  if (set_dev(c)) return -2;
  if (int rc = ensure_side_factors(c, side)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  SideBuf& sb = c->s[side];
  const size_t n = (size_t)sb.n, kp = c->kp, k = c->k;
  return with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    std::vector<T> h(n * kp);
    HIPCHK(scopy(c, h.data(), sb.F, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < n; ++r)
      for (size_t j = 0; j < k; ++j) f[r * k + j] = h[r * kp + j];
    return 0;
  });
}

int qmfx_fill_uniform(qmfx_ctx* c, int side, double bound, uint64_t seed) {
  if (set_dev(c)) return -2;
  if (int rc = ensure_side_factors(c, side)) return rc;
  SideBuf& sb = c->s[side];
  return with_prec(c->prec, [&](auto t) {
    using T = decltype(t);
    HIPCHK(launch_fill_uniform(sb.F.as<T>(), sb.n, c->kp, c->k, bound, seed, c->stream));
    return 0;
  });
}

// ---- measurement ---------------------------------------------------------------------------
int qmfx_solve_kernel_stats(qmfx_ctx* c, double* total_ms, int64_t* launches, double* flops,
                            double* bytes) {
  return c->solve.get(total_ms, launches, flops, bytes);
}

int qmfx_kernel_stats(qmfx_ctx* c, int cls, double* total_ms, int64_t* launches, double* flops,
                      double* bytes) {
  if (cls < 0 || cls > 2) return fail("class must be 0 (direct), 1 (whitened) or 2 (half)");
  return c->cls[cls].get(total_ms, launches, flops, bytes);
}

int qmfx_kernel_stats_side(qmfx_ctx* c, int cls, int side, double* total_ms, int64_t* launches,
                           double* flops, double* bytes) {
  if (cls < 0 || cls > 2) return fail("class must be 0 (direct), 1 (whitened) or 2 (half)");
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  return c->side[side][cls].get(total_ms, launches, flops, bytes);
}

int qmfx_reset_stats(qmfx_ctx* c) {
  for (int sd = 0; sd < 2; ++sd) {
    c->xch_ms[sd] = c->xch_tail_ms[sd] = c->xch_solve_ms[sd] = 0;
    c->xch_halves[sd] = 0;
  }
  c->solve = KernelStat{};
  for (int i = 0; i < 3; ++i) c->cls[i] = c->side[0][i] = c->side[1][i] = KernelStat{};
  return 0;
}

int qmfx_exchange_stats(qmfx_ctx* c, int side, double* exchange_ms, double* exposed_ms,
                        double* solve_ms, int64_t* halves) {
  if (side != 0 && side != 1) return fail("side must be 0 or 1");
  if (exchange_ms) *exchange_ms = c->xch_ms[side];
  if (exposed_ms) *exposed_ms = c->xch_tail_ms[side];
  if (solve_ms) *solve_ms = c->xch_solve_ms[side];
  if (halves) *halves = c->xch_halves[side];
  return 0;
}

// A timing-variant build (tools/build_variant.sh) links an object that defines this; the
// product library does not, and reports "".
extern "C" __attribute__((weak)) const char* qmfx_variant_flags_tag(void);
const char* qmfx_build_variant(void) { return qmfx_variant_flags_tag ? qmfx_variant_flags_tag() : ""; }

int qmfx_selftest_mfma(int device, int precision, const double* A, const double* B, double* C) {
  HIPCHK(hipSetDevice(device));
  return with_prec(precision, [&](auto t) {
    using T = decltype(t);
    DevPtr<T> dA, dB, dC;
    HIPCHK(dev_alloc(dA, 64 * sizeof(T)));
    HIPCHK(dev_alloc(dB, 64 * sizeof(T)));
    HIPCHK(dev_alloc(dC, 256 * sizeof(T)));
    const auto a = convert<T>(A, 64), b = convert<T>(B, 64);
    HIPCHK(hipMemcpy(dA, a.data(), 64 * sizeof(T), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dB, b.data(), 64 * sizeof(T), hipMemcpyHostToDevice));
    HIPCHK(launch_mfma_selftest(dA, dB, dC, nullptr));
    std::vector<T> cc(256);
    HIPCHK(hipMemcpy(cc.data(), dC, 256 * sizeof(T), hipMemcpyDeviceToHost));
    std::copy(cc.begin(), cc.end(), C);
    return 0;
  });
}

}  // extern "C"
