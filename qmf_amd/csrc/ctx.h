// Internal header of the host units behind the C ABI (api_*.cpp; include/qmfx.h is the
// installed one): the context and its per-side buffers, error reporting, the precision
// dispatch and the helpers the units share.
#pragma once
#include "../../include/qmfx.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"

#define QMFX_MAX_PIECES 16

namespace qmfx {

constexpr int kHalfStatus = 1024;  // dsum offset of the end-of-half status block

// message of the last failing call on this thread (qmfx_last_error); defined in api_ctx.cpp
extern thread_local std::string g_err;

inline int fail(const std::string& m, int code = -1) {
  g_err = m;
  return code;
}

#define HIPCHK(x)                                                                            \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess)                                                                    \
      return qmfx::fail(std::string(#x) + ": " + hipGetErrorString(e_), -2);                 \
  } while (0)

#define NCCLCHK(x)                                                                           \
  do {                                                                                       \
    ncclResult_t r_ = (x);                                                                   \
    if (r_ != ncclSuccess)                                                                   \
      return qmfx::fail(std::string(#x) + ": " + ncclGetErrorString(r_), -3);                \
  } while (0)

// kernel time and algorithmic work of one class of launches since qmfx_reset_stats
struct KernelStat {
  double ms = 0;
  int64_t launches = 0;
  double flops = 0, bytes = 0;
  void add(double m, double fl, double by) {
    ms += m;
    launches += 1;
    flops += fl;
    bytes += by;
  }
  int get(double* m, int64_t* n, double* fl, double* by) const {
    if (m) *m = ms;
    if (n) *n = launches;
    if (fl) *fl = flops;
    if (by) *by = bytes;
    return 0;
  }
};

// Solve pieces: a rank's rows split into nnz-balanced contiguous sub-ranges, each with its
// own section of the order list laid out like the side's (ord + wb[i] relative).  With
// several ranks, piece j of every rank is all-gathered while piece j+1 is solved.
struct Piece {
  int64_t rb = 0, re = 0, ord = 0, n_ord = 0;
  int64_t wb[kMaxNTN + 1] = {};
  // split-K heavy rows (the first nh direct slots): heavy indices h0 .. h0+nh, segments
  // s0 .. s0+ns (of the side's d_seg / d_heavy / d_hseg lists)
  int64_t nh = 0, h0 = 0, s0 = 0, ns = 0;
};

struct SideBuf {
  int64_t n = 0;
  int64_t nnz = 0;
  DevPtr<int64_t> rowptr;
  DevPtr<int32_t> col;
  DevPtr<void> val;
  DevPtr<void> F;
  std::vector<int64_t> h_rowptr;
  std::vector<int64_t> h_ids;           // ascending ids (only when built by qmfx_group_signals)
  int64_t rbeg = 0, rend = 0;           // rows solved by this rank
  // With several ranks the CSR keeps only this rank's rows (signals rowptr[rbeg] ..
  // rowptr[rend]); col/val point at that shard and shard_off = rowptr[rbeg], so kernels
  // index them with the global rowptr through colp()/valp().
  int64_t shard_off = 0;
  bool sharded = false;
  std::vector<int64_t> bounds;          // per-rank row boundaries (world+1)
  // Row buckets of this rank (device list `order`): [whitened n≤16 | ≤32 | … | ≤16·kMaxNTN |
  // direct rows, heaviest first].  wb[i]..wb[i+1] = whitened bucket NTN = i+1;
  // wb[kMaxNTN]..n_ord = direct.  nnz per bucket class for the roofline accounting.
  DevPtr<int64_t> d_order;
  DevPtr<RowDesc> d_desc;  // per slot of d_order: CSR range and row
  int64_t wb[kMaxNTN + 1] = {};
  int64_t n_ord = 0;
  double nnz_w = 0, nnz_d = 0;
  double flops_w = 0;  // algorithmic flops of the whitened rows per half (see half_end)
  bool buckets_valid = false;
  std::vector<Piece> pieces;
  std::vector<int64_t> pbounds;  // world × (npieces + 1): piece boundaries of every rank
  // split-K heavy rows of this rank: per segment {CSR begin, signals, heavy index}; per heavy
  // row {first segment, 0, row} (the seg_mode 2 solve) and the segment prefix hseg[nh+1]
  DevPtr<RowDesc> d_seg, d_heavy;
  DevPtr<int64_t> d_hseg;
  int64_t nseg = 0, nheavy = 0;
};

// Scratch of the top-N selection (RecArgs; topn_* below): the uploaded request rows, one
// batch's rows in double, the per-chunk survivor lists and the outputs; the deny bitmap of
// qmfx_recommend_without; the lists and work items of qmfx_recommend_candidates (CandArgs).
struct TopN {
  Scratch<int64_t> users, items;
  Scratch<double> udbl, pscore, scores;
  Scratch<int32_t> pitem, pcnt, counts;
  Scratch<unsigned long long> deny;
  Scratch<int32_t> cand, wuser;
  Scratch<int64_t> cptr, woff;
};

// Scratch of the screened top-N (qmfx_recommend_screened): the requested rows gathered, the f32
// copies of an fp64 context's rows, both sides' norms, the thresholds, pass counters and kept
// lists, the sort keys, and the exact-scan users with their outputs.
struct Screen {
  Scratch<void> ug;                  // [nreq][kp] context precision
  Scratch<float> uf, itf;            // fp64 contexts: [nreq][kp], [nitems][kp]
  Scratch<double> unorm, inorm, thr;
  Scratch<int32_t> cnt, scnt, list;
  Scratch<uint64_t> keys, keys2;
  Scratch<int64_t> xusers, xitems;
  Scratch<double> xscores;
  Scratch<int32_t> xcounts;
  Event ev[7];                       // stage boundaries (created by the first call)
  int64_t stats[4] = {0, 0, 0, 0};   // qmfx_recommend_screen_stats
  double stage_ms[6] = {0, 0, 0, 0, 0, 0};  // qmfx_recommend_screen_stage_ms
};

}  // namespace qmfx

// Members are destroyed last to first: the streams stand first, so they outlive every buffer
// and event that work enqueued on them may use.
struct qmfx_ctx {
  qmfx::Stream stream;
  qmfx::Stream comm_stream;  // collectives (created by qmfx_dist_init*)
  int device = 0;
  int prec = 32;
  int k = 0, kp = 0, nt = 0;
  size_t esz = 4;
  int cus = 0;  // compute units of the device
  qmfx::SideBuf s[2];
  int64_t nnz = 0;
  qmfx::DevPtr<void> G;
  qmfx::DevPtr<double> gpart;
  int gpart_blocks = 1024;
  qmfx::DevPtr<double> rowloss;
  int64_t rowloss_cap = 0;
  qmfx::DevPtr<int32_t> status;
  // pivoted re-solve of flagged rows (fallback.hip): scratch and [re-solved, singular] counts
  qmfx::DevPtr<double> fb_scratch;
  qmfx::DevPtr<unsigned long long> fb_cnt;
  int64_t fb_rows = 0;  // rows re-solved by the last half
  qmfx::DevPtr<double> dsum;
  qmfx::PinnedPtr<double> hsum;
  qmfx::Event ev0, ev1;
  int last_side = 0;
  // distributed
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  // BPR
  qmfx::DevPtr<int64_t> pos_user;
  qmfx::DevPtr<int32_t> pos_item;
  int64_t npos = 0;
  int64_t max_user_pos = 0;  // largest positive count of one user (Hogwild collision estimate)
  qmfx::DevPtr<int64_t> urowptr;
  qmfx::DevPtr<int32_t> uitems;
  qmfx::DevPtr<void> bias;
  qmfx::DevPtr<int32_t> bad;
  qmfx::DevPtr<int64_t> trip[2];
  int64_t trip_n[2] = {0, 0};
  const void* trip_src[2] = {nullptr, nullptr};
  qmfx::DevPtr<double> eval_partial;
  // test-set evaluation (qmfx_eval_set_labels / qmfx_eval_ranks)
  int64_t ev_ntest = 0, ev_nlab = 0, ev_npos = 0, ev_chunks = 0;
  qmfx::DevPtr<int64_t> ev_users;
  qmfx::DevPtr<int32_t> ev_slot;
  qmfx::DevPtr<int64_t> ev_item, ev_pidx, ev_pptr;
  qmfx::DevPtr<double> ev_lscore, ev_pscore;
  qmfx::DevPtr<unsigned long long> ev_above;
  qmfx::DevPtr<double> ev_sq, ev_udbl;
  // The serving calls' scratch: every buffer knows the bytes it holds and is grown on demand
  // (reserve).  Top-N selection (qmfx_recommend, qmfx_similar, qmfx_recommend_fold_in):
  qmfx::TopN rc;
  qmfx::Screen scr;
  // rows given with a call as a CSR of their own (fold-in, qmfx_wals_explain_rows): the last
  // upload (upload_rows, rows.h)
  qmfx::Scratch<int64_t> fr_rowptr;
  qmfx::Scratch<int32_t> fr_col;
  qmfx::Scratch<void> fr_val;
  // fold-in (qmfx_wals_fold_in, qmfx_recommend_fold_in): the uploaded rows' plan and their own
  // output rows, row losses and status words.  fi_classes / fi_n: the last fold-in's plan.
  qmfx::Scratch<void> fi_X;
  qmfx::Scratch<double> fi_rowloss;
  qmfx::Scratch<int32_t> fi_status;
  qmfx::Scratch<uint64_t> fi_keys, fi_keys2;
  qmfx::Scratch<int64_t> fi_order;
  qmfx::Scratch<qmfx::RowDesc> fi_desc;
  qmfx::Scratch<int64_t> fi_wb;
  qmfx::Scratch<double> fi_out;
  // BPR fold-in (qmfx_bpr_fold_in, qmfx_bpr_recommend_fold_in) shares fr_rowptr / fr_col, fi_X,
  // fi_rowloss and fi_out; its own: the passes' learning rates in the context precision
  qmfx::Scratch<void> fi_lr;
  int64_t fi_classes[qmfx::kMaxNTN + 3] = {};
  int64_t fi_n = -1;  // rows of the last plan (-1: no fold-in yet)
  // explanations (qmfx_wals_explain, qmfx_wals_explain_rows): the uploaded queries, the
  // outputs and the KP > 128 factor scratch
  qmfx::Scratch<int64_t> ex_rows, ex_qptr, ex_targets, ex_allq, ex_sources, ex_positions;
  qmfx::Scratch<double> ex_contribs, ex_totals, ex_all, ex_scratch;
  qmfx::Scratch<int32_t> ex_counts;
  qmfx::Scratch<unsigned long long> ex_first;
  // similar rows (qmfx_similar, qmfx_factor_norms): one side's row norms, written by every call
  qmfx::Scratch<double> sim_norms;
  uint64_t bpr_epochs = 0;
  // QMFX_FAULT_COMM_RANK=<rank>[:<after>] (tests), read once at create: that rank's piece
  // broadcasts fail as if RCCL had failed once <after> of them have succeeded (-1: none)
  int fault_comm_rank = -1;
  int64_t fault_comm_after = 0, comm_pieces_done = 0;
  bool whitened_enabled = true;  // QMFX_NO_WHITEN=1 forces the direct kernel for every row
  int wb_k64_ntn = 0;            // QMFX_WB_K64_NTN: largest whitened bucket at k = 64 (0: default)
  // the half-epoch in progress (qmfx_wals_half's phases)
  struct HalfStateT {
    int side = 0;
    double alpha = 0, lambda = 0;
    bool use_w = false;
    int64_t nD = 0;
    const char* trace_path = nullptr;
  } hs;
  // split-K heavy rows (direct and multi-wave tilings): rows with more than heavy_min signals are
  // cut into segments of seg_len (QMFX_HEAVY_MIN / QMFX_SEG_LEN, read once at create;
  // heavy_min 0 = off); partials [segments][NTT·256 + KP] in the context precision + Σc/flag
  int64_t heavy_min = 16384;
  int64_t seg_len = 8192;
  qmfx::DevPtr<void> part, partb;
  qmfx::DevPtr<double> partc;
  int64_t part_cap = 0;  // segments
  // whitened path buffers
  qmfx::DevPtr<void> Z;  // whitened fixed side [max(nu, ni)][kp]
  int64_t z_cap = 0;
  qmfx::DevPtr<void> Linv;  // kp × kp
  qmfx::DevPtr<int32_t> chol_status;
  qmfx::DevPtr<double> chol_scratch;  // KP > 128: the fp64 factorization of G + λI (global)
  qmfx::DevPtr<void> Gimg;  // G + λI as the direct kernel's accumulator-tile image
  qmfx::DevPtr<uint64_t> trace;  // QMFX_TRACE diagnostics: whitened-row phase timestamps
  int64_t trace_cap = 0;
  // whole-half timing: [0] start, [2] end
  qmfx::Event evh[4];
  // solve pieces per half (QMFX_PIECES; default 1 on one rank, 8 with several: the last
  // piece's all-gather is the exposed part) and their
  // events: [piece][start, direct done, whitened done]; collectives run on comm_stream
  int npieces = 0;
  qmfx::Event evp[QMFX_MAX_PIECES][3];
  qmfx::Event ev_sum, ev_comm;
  // multi-rank halves: per piece, the collective stream's [start, end] of its broadcasts
  // (start = when the stream reached them: the piece's solves done and the previous piece's
  // broadcasts finished); per solved side since reset: Σ broadcast time, the exposed tail
  // (last piece's solves done → its broadcasts done) and Σ solve time of the pieces
  qmfx::Event evx[QMFX_MAX_PIECES][2];
  double xch_ms[2] = {0, 0}, xch_tail_ms[2] = {0, 0}, xch_solve_ms[2] = {0, 0};
  int64_t xch_halves[2] = {0, 0};
  // BPR launch plan of the last epoch (qmfx_bpr_plan)
  int bpr_waves = 0, bpr_atomic_user = 0;
  // row solves of every half and BPR epoch; per class: 0 direct kernel, 1 whitened kernels
  // (row solve + unwhiten), 2 whole half; and the classes per solved side (a class's launches
  // differ by side: at C3 the direct kernel takes 187 ms in the item half and 69 µs in the
  // user half)
  qmfx::KernelStat solve, cls[3], side[2][3];
  // set when qmfx_wals_half_multi aborted the clique after a failed collective
  bool comm_aborted = false;
};

namespace qmfx {

// Runs f with a value of the factor type: with_prec(c->prec, [&](auto t) { using T =
// decltype(t); … }).  The one place where the precision becomes a type.
template <typename F>
auto with_prec(int prec, F&& f) {
  return prec == 32 ? f(float{}) : f(double{});
}

inline int set_dev(qmfx_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  return 0;
}

// Every transfer goes through the context's (non-blocking) stream so it is ordered with the
// kernels and async memsets issued there; the call returns when the copy has completed.
inline hipError_t scopy(qmfx_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (bytes == 0) return hipSuccess;
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(c->stream);
}

template <typename T>
std::vector<T> convert(const double* src, size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (T)src[i];
  return v;
}

// host doubles → a device array in the context precision, and back
inline hipError_t copy_in(qmfx_ctx* c, void* dst, const double* src, size_t n) {
  if (c->prec == 64) return scopy(c, dst, src, n * 8, hipMemcpyHostToDevice);
  const auto v = convert<float>(src, n);
  return scopy(c, dst, v.data(), n * 4, hipMemcpyHostToDevice);
}
inline hipError_t copy_out(qmfx_ctx* c, double* dst, const void* src, size_t n) {
  if (c->prec == 64) return scopy(c, dst, src, n * 8, hipMemcpyDeviceToHost);
  std::vector<float> v(n);  // the device holds floats; widen exactly
  const hipError_t e = scopy(c, v.data(), src, n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) std::copy(v.begin(), v.end(), dst);
  return e;
}

// scratch grown on demand: keeps the buffer when it already holds `bytes`
template <typename T>
int reserve(Scratch<T>& p, size_t bytes) {
  if (p && p.bytes >= bytes) return 0;
  p.bytes = 0;
  HIPCHK(dev_alloc(p, bytes));
  p.bytes = bytes;
  return 0;
}

// The top-N selection's scratch for nreq request rows and `lists` per-chunk survivor lists.
inline int topn_reserve_lists(qmfx_ctx* c, int64_t nreq, size_t lists, int topn) {
  TopN& s = c->rc;
  const size_t n = (size_t)nreq, out = n * (size_t)topn;
  if (int rc = reserve(s.users, n * 8)) return rc;
  if (int rc = reserve(s.items, out * 8)) return rc;
  if (int rc = reserve(s.udbl, (size_t)(eval_user_rows(nreq) * c->k) * 8)) return rc;
  if (int rc = reserve(s.pscore, lists * (size_t)topn * 8)) return rc;
  if (int rc = reserve(s.scores, out * 8)) return rc;
  if (int rc = reserve(s.pitem, lists * (size_t)topn * 4)) return rc;
  if (int rc = reserve(s.pcnt, lists * 4)) return rc;
  return reserve(s.counts, n * 4);
}
// ... over all ncand candidate rows (the dense scan's chunks)
inline int topn_reserve(qmfx_ctx* c, int64_t nreq, int64_t ncand, int topn) {
  return topn_reserve_lists(c, nreq, (size_t)(eval_chunks(nreq, ncand) * eval_user_rows(nreq)),
                            topn);
}
// What every selection sets the same way (SimArgs derives from RecArgs); the caller adds
// U, I and what is its own.
template <typename T>
void topn_args(qmfx_ctx* c, RecArgs<T>& a, int64_t nreq, int64_t ncand, int topn) {
  const TopN& s = c->rc;
  a.users = s.users;
  a.nreq = nreq;
  a.nitems = ncand;
  a.k = c->k;
  a.kp = c->kp;
  a.topn = topn;
  a.udbl = s.udbl;
  a.part_score = s.pscore;
  a.part_item = s.pitem;
  a.part_cnt = s.pcnt;
  a.items = s.items;
  a.scores = s.scores;
  a.counts = s.counts;
}
inline int topn_copy_out(qmfx_ctx* c, int64_t nreq, int topn, int64_t* items, double* scores,
                         int32_t* counts) {
  const TopN& s = c->rc;
  const size_t out = (size_t)nreq * (size_t)topn;
  HIPCHK(scopy(c, items, s.items, out * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, scores, s.scores, out * 8, hipMemcpyDeviceToHost));
  HIPCHK(scopy(c, counts, s.counts, (size_t)nreq * 4, hipMemcpyDeviceToHost));
  return 0;
}
// A selection's work for qmfx_solve_kernel_stats: one unit = one request × candidate score,
// 2k flop; bytes: the candidates' factors once per group of 32 requests.
inline double topn_flops(const qmfx_ctx* c, int64_t nreq, int64_t ncand) {
  return 2.0 * (double)nreq * (double)ncand * c->k;
}
inline double topn_bytes(const qmfx_ctx* c, int64_t nreq, int64_t ncand) {
  return (double)((nreq + 31) / 32) * (double)ncand * c->k * (double)c->esz;
}

// api_recommend.cpp, shared with api_screened.cpp: what every recommend call rejects before it
// touches the device, and qmfx_recommend with the ndeny items of `deny` eligible for nobody
int rec_check(const qmfx_ctx* c, int64_t nusers, const int64_t* users, int topn, int exclude,
              int use_biases);
int recommend_dense(qmfx_ctx* c, int64_t nusers, const int64_t* users, int64_t ndeny,
                    const int64_t* deny, int topn, int exclude, int use_biases, int64_t* items,
                    double* scores, int32_t* counts);

// col/val as the kernels index them: with the global rowptr (see SideBuf::shard_off)
inline int32_t* colp(const SideBuf& sb) { return sb.col - sb.shard_off; }
template <typename T>
const T* valp(const SideBuf& sb) {
  return sb.val.as<T>() - sb.shard_off;
}

// The factors, biases and seen lists of a recommend call.
template <typename T>
void rec_model(const qmfx_ctx* c, RecArgs<T>& a, int exclude, int use_biases) {
  const SideBuf& su = c->s[0];
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
}

inline int ensure_side_factors(qmfx_ctx* c, int side) {
  SideBuf& sb = c->s[side];
  if (sb.F) return 0;
  if (sb.n <= 0) return fail("shape not set (qmfx_set_shape)");
  // one extra all-zero row (index n): padding signals of the row kernels gather it
  HIPCHK(dev_alloc(sb.F, (size_t)(sb.n + 1) * c->kp * c->esz));
  HIPCHK(hipMemsetAsync(sb.F, 0, (size_t)(sb.n + 1) * c->kp * c->esz, c->stream));
  return 0;
}

// item biases (BPR), zero until set
inline int ensure_bias(qmfx_ctx* c) {
  if (c->bias) return 0;
  HIPCHK(dev_alloc(c->bias, (size_t)c->s[1].n * c->esz));
  HIPCHK(hipMemsetAsync(c->bias, 0, (size_t)c->s[1].n * c->esz, c->stream));
  return 0;
}

// YᵀY on the tiled multi-wave kernel (fp32 k > 128, fp64 k > 64)
inline bool use_big(const qmfx_ctx* c) { return c->nt >= big_gram_min_nt(c->prec == 32 ? 4 : 8); }
static_assert(big_gram_min_nt(4) == 8 + 1 && big_gram_min_nt(8) == 4 + 1,
              "launch_gram builds the one-wave YᵀY up to nt = 8 (fp32) and 4 (fp64)");
// direct rows on the multi-wave row kernel: k > 128 (fp64 k = 80..128 runs the one-wave
// direct kernel with its accumulators across the VGPR + AGPR file; the
// multi-wave kernel at fp64 k = 128 measured 213.7 ms per C3 item half at four waves per row
// and 206.5 ms at two, against 179.2 / 175.6 ms here: round 6, profiles/r06/ab_big128_c3_f64.txt)
inline bool use_big_rows(const qmfx_ctx* c) { return c->nt >= kBigRowMinNT; }
static_assert(kBigRowMinNT == 8 + 1, "launch_wals_direct builds the one-wave rows up to nt = 8");

// Largest whitened-row bucket (NTN: n ≤ 16·NTN) for this factor tiling: n ≤ KP/2
// and ≤ 64, except on the streamed kernels' two-signals-per-lane buckets: fp32 k = 128 / 256
// up to n = 128, fp64 k = 128 / 256 up to n = 80 (n = 81..96 spilled 64 VGPRs; those rows stay
// direct).
constexpr int default_whitened_ntn(int elem_bytes, int nt) {
  if (elem_bytes == 4) {
    if (nt == 8 || nt == 16) return 8;
    if (nt > 8) return 0;  // fp32 k = 144..240: every row on the big k×k kernel
    // k = 64: n ≤ 64 (C2 same-box A/Bs, round 5: n ≤ 32 → n ≤ 48 10.0 → 9.1 ms/epoch, → n ≤ 64
    // 8.7 → 8.2)
    if (nt == 4) return 4;
    return nt / 2 < 4 ? nt / 2 : 4;
  }
  if (nt == 8 || nt == 16) return 5;
  if (nt > 8) return 0;
  // k = 64: n ≤ 48 on the streamed fp64 kernel (C2 fp64 same-box A/B, round 5: 18.5 → 17.6
  // ms/epoch; n ≤ 64 measured no better)
  if (nt == 4) return 3;
  return nt / 2 < 4 ? nt / 2 : 4;
}
// the policy never asks for a bucket without a kernel (wb_max_ntn, kernels.h)
constexpr bool whitened_defaults_have_kernels() {
  for (int nt = 1; nt <= 16; ++nt)
    for (int eb = 4; eb <= 8; eb += 4)
      if (default_whitened_ntn(eb, nt) > wb_max_ntn(eb, nt)) return false;
  return true;
}
static_assert(whitened_defaults_have_kernels());
inline int max_whitened_ntn(const qmfx_ctx* c) {
  if (!c->whitened_enabled) return 0;
  const int eb = c->prec == 32 ? 4 : 8;
  const int want = c->nt == 4 && c->wb_k64_ntn > 0 ? c->wb_k64_ntn : default_whitened_ntn(eb, c->nt);
  return std::min(want, wb_max_ntn(eb, c->nt));
}

inline int npieces(const qmfx_ctx* c) {
  if (c->npieces > 0) return c->npieces;
  return c->world > 1 ? 8 : 1;
}

// YᵀY of a side's factors into c->G (full replica on every rank)
template <typename T>
hipError_t launch_gram_t(qmfx_ctx* c, const SideBuf& R) {
  return use_big(c) ? launch_gram_big(R.F.as<T>(), R.n, c->nt, c->G.as<T>(), c->gpart,
                                      c->gpart_blocks, c->stream)
                    : launch_gram(R.F.as<T>(), R.n, c->nt, c->G.as<T>(), c->gpart,
                                  c->gpart_blocks, c->stream);
}

// api_signals.cpp
void drop_csr(SideBuf& sb);  // releases the CSR arrays of a side
void set_default_bounds(SideBuf& sb, int world, int rank);
void plan_pieces(const std::vector<int64_t>& rp, const std::vector<int64_t>& bounds, int world,
                 int P, std::vector<int64_t>& pb);
int build_buckets(qmfx_ctx* c, int side);
int shard_csr(qmfx_ctx* c, SideBuf& sb);

// api_eval.cpp
void drop_eval_labels(qmfx_ctx* c);  // releases the test-label set (qmfx_eval_ranks then fails)
// api_bpr.cpp
void drop_bpr_positives(qmfx_ctx* c);  // releases the positives (qmfx_bpr_epoch then fails)
extern const char* const kBadGradients;  // the message of a non-finite loss derivative (-4)

}  // namespace qmfx
