// Kernel argument structs and host launchers shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "own.h"

namespace qmfx {

// Per-slot row descriptor of a side's processing order (built once with the buckets):
// the CSR range of the row and the row itself, so a persistent row kernel reaches a row's
// signals in one dependent load instead of order → rowptr → signals.
struct RowDesc {
  int64_t beg;
  int32_t n;
  int32_t row;
};

template <typename T>
struct SolveArgs {
  const int64_t* rowptr;  // CSR of the side being solved
  const int32_t* col;     // column = row index on the fixed side
  const T* val;           // raw interaction value v
  const T* Y;             // fixed-side factors [nY][KP]
  const T* G;             // YᵀY, KP×KP
  T* X;                   // solved-side factors [nX][KP]
  double* rowloss;        // [nX]
  int32_t* status;        // [nX] non-zero: non-positive pivot (system not SPD)
  const int64_t* order;   // optional processing order (nullptr = identity)
  int64_t row_begin;      // first slot of the order handled by this launch
  int64_t nrows;          // number of rows (blocks)
  T alpha;
  T lambda;
  int k;                  // real number of factors (≤ KP)
  const RowDesc* desc;    // per-slot descriptors (persistent row kernels; indexed like order)
  const T* Gimg;          // direct kernel: G + λI as per-lane accumulator tiles (gimg_kernel)
  uint64_t* trace;        // diagnostics only (QMFX_TRACE): per-slot phase timestamps
  int32_t zrow;           // whitened kernel: index of an all-zero row of Y (padding signals)
  // Heavy rows (split-K, direct kernel only): rows with more than `heavy_min` signals are cut
  // into segments; seg_mode 1 accumulates one segment's Gram (slot = segment) into
  // part/partb/partc, heavy_reduce_kernel sums a row's segments in fp64 (fixed order) into
  // its first segment's slot, and seg_mode 2 solves the row from there (desc.beg = that
  // slot, desc.n = 0).  seg_mode 0 is the ordinary row solve.
  int seg_mode;
  T* part;                // [segments][NTT·256] accumulator-tile images
  T* partb;               // [segments][KP] right-hand sides
  double* partc;          // [segments][2]: Σc, negative-weight flag
};

// Heavy-row partial reduction: for heavy rows h0 .. h0+nh, segments hseg[h] .. hseg[h+1] are
// summed (fp64, fixed order) with G + λI into segment hseg[h]'s slot.
hipError_t launch_heavy_reduce(float* part, float* partb, double* partc, const int64_t* hseg,
                               int64_t h0, int64_t nh, const float* Gimg, int nt, hipStream_t s);
hipError_t launch_heavy_reduce(double* part, double* partb, double* partc, const int64_t* hseg,
                               int64_t h0, int64_t nh, const double* Gimg, int nt, hipStream_t s);

// The same for the multi-wave k > 128 tilings (the rows of wals_big.hip; in wals_heavy.hip too):
// builds G + λI's tile image in Gimg first (runtime tile count, no column permutation).
hipError_t launch_heavy_reduce_big(float* part, float* partb, double* partc, const int64_t* hseg,
                                   int64_t h0, int64_t nh, const float* G, float* Gimg, int nt,
                                   int k, double lambda, hipStream_t s);
hipError_t launch_heavy_reduce_big(double* part, double* partb, double* partc, const int64_t* hseg,
                                   int64_t h0, int64_t nh, const double* G, double* Gimg, int nt,
                                   int k, double lambda, hipStream_t s);

// Per-row kernels take one workgroup per row (slot = row_begin + blockIdx.x).  A launch's
// total thread count must fit 32 bits (10M rows × 512 threads does not), so rows go out in
// chunks of at most 2^31 / threads workgroups.
// (QMFX_ROW_CHUNK lowers the chunk for the tests.)
template <typename T, typename F>
hipError_t launch_row_chunks(const SolveArgs<T>& a, int threads, F launch) {
  int64_t cap = ((int64_t)1 << 31) / threads;
  if (const char* e = std::getenv("QMFX_ROW_CHUNK"))
    if (std::atoll(e) > 0 && std::atoll(e) < cap) cap = std::atoll(e);
  for (int64_t done = 0; done < a.nrows; done += cap) {
    SolveArgs<T> c = a;
    c.row_begin = a.row_begin + done;
    c.nrows = a.nrows - done < cap ? a.nrows - done : cap;
    launch(c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// G + λI (padding diagonal 1) → the direct row kernel's accumulator-tile image
hipError_t launch_gimg(const float* G, int nt, int k, double lambda, float* img, hipStream_t s);
hipError_t launch_gimg(const double* G, int nt, int k, double lambda, double* img, hipStream_t s);

hipError_t launch_wals_direct(const SolveArgs<float>& a, int nt, hipStream_t s);
hipError_t launch_wals_direct(const SolveArgs<double>& a, int nt, hipStream_t s);
// seg_mode 1 / 2 of the direct kernel (wals_heavy.hip; launch_wals_direct forwards there)
hipError_t launch_wals_heavy(const SolveArgs<float>& a, int nt, hipStream_t s);
hipError_t launch_wals_heavy(const SolveArgs<double>& a, int nt, hipStream_t s);
// Multi-wave kernels for large factor counts, up to k = 256: the tilings each is built for
// (ctx.h use_big_rows / use_big send exactly these there).  Row solve (wals_big.hip): k > 128.
// Tiled YᵀY (gram_big.hip): fp32 k > 128, fp64 k > 64.
constexpr int kBigMaxNT = 16;
constexpr int kBigRowMinNT = 9;
constexpr int big_gram_min_nt(int elem_bytes) { return elem_bytes == 4 ? 9 : 5; }
static_assert(big_gram_min_nt(4) <= kBigRowMinNT && big_gram_min_nt(8) <= kBigRowMinNT,
              "a side on the multi-wave row kernel takes its YᵀY from the tiled kernel");
hipError_t launch_wals_big(const SolveArgs<float>& a, int nt, hipStream_t s);
hipError_t launch_wals_big(const SolveArgs<double>& a, int nt, hipStream_t s);
hipError_t launch_gram_big(const float* Y, int64_t n, int nt, float* G, double* partial,
                           int max_blocks, hipStream_t s);
hipError_t launch_gram_big(const double* Y, int64_t n, int nt, double* G, double* partial,
                           int max_blocks, hipStream_t s);
// whitened-row buckets: n ≤ 16·NTN, NTN = 1..kMaxNTN
constexpr int kMaxNTN = 8;
// The largest bucket that has a whitened row kernel for factor tiling nt (KP = 16·nt), 0 for
// none: n ≤ KP/2 and ≤ 64, except k = 64 (n ≤ 64) and the two-signals-per-lane buckets of
// k = 128 / 256 (fp32 n ≤ 128, fp64 n ≤ 80).  launch_wals_woodbury builds exactly these.
constexpr int wb_max_ntn(int elem_bytes, int nt) {
  if (nt == 8 || nt == 16) return elem_bytes == 4 ? 8 : 5;
  if (nt < 2 || nt > 8) return 0;
  return nt == 4 ? 4 : nt / 2;
}
static_assert(wb_max_ntn(4, 16) <= kMaxNTN && wb_max_ntn(8, 16) <= kMaxNTN);
hipError_t launch_wals_woodbury(const SolveArgs<float>& a, int nt, int ntn, hipStream_t s);
hipError_t launch_wals_woodbury(const SolveArgs<double>& a, int nt, int ntn, hipStream_t s);
// cus: compute units of the device (sizes the persistent grid)
hipError_t launch_whiten(const float* in, float* out, const int64_t* order, int64_t nrows,
                         int nt, const float* Linv, double* rowloss, double lambda,
                         bool unwhiten, int cus, hipStream_t s);
hipError_t launch_whiten(const double* in, double* out, const int64_t* order, int64_t nrows,
                         int nt, const double* Linv, double* rowloss, double lambda,
                         bool unwhiten, int cus, hipStream_t s);
// scratch: KP·(KP+1) doubles, used when KP > 128 (the fp64 matrix does not fit LDS)
hipError_t launch_chol_inv(const float* G, int nt, int k, double lambda, float* Linv,
                           int32_t* status, double* scratch, hipStream_t s);
hipError_t launch_chol_inv(const double* G, int nt, int k, double lambda, double* Linv,
                           int32_t* status, double* scratch, hipStream_t s);
hipError_t launch_gram(const float* Y, int64_t n, int nt, float* G, double* partial,
                       int max_blocks, hipStream_t s);
hipError_t launch_gram(const double* Y, int64_t n, int nt, double* G, double* partial,
                       int max_blocks, hipStream_t s);
hipError_t launch_sum_f64(const double* x, int64_t n, double* out, hipStream_t s);
hipError_t launch_mfma_selftest(const float* A, const float* B, float* C, hipStream_t s);
hipError_t launch_mfma_selftest(const double* A, const double* B, double* C,
                                hipStream_t s);

// Pivoted fp64 re-solve of the rows flagged in `status` (fallback.hip)
template <typename T>
struct FallbackArgs {
  const int64_t* rowptr;
  const int32_t* col;
  const T* val;
  const T* Y;             // fixed side [nY][kp]
  const T* G;             // YᵀY of the fixed side, kp×kp
  T* X;                   // solved side [nX][kp]
  double* rowloss;
  int32_t* status;        // in: non-zero = flagged; out: 1 re-solved, 2 singular
  const RowDesc* desc;    // slot → row
  int64_t slot_begin, nslots;
  double alpha, lambda;
  int k, kp;
  double* scratch;        // FB_MAX_GRID × (kp + 3) × kp doubles
  unsigned long long* counters;  // [0] rows re-solved, [1] singular rows
};
constexpr int FB_MAX_GRID = 64;
hipError_t launch_wals_fallback(const FallbackArgs<float>& a, hipStream_t s);
hipError_t launch_wals_fallback(const FallbackArgs<double>& a, hipStream_t s);
// out: A (k×k row-major, λ included), then b (k), then Σc — one row's system
hipError_t launch_wals_system(const FallbackArgs<float>& a, int64_t beg, int64_t end, double* out,
                              hipStream_t s);
hipError_t launch_wals_system(const FallbackArgs<double>& a, int64_t beg, int64_t end,
                              double* out, hipStream_t s);

// Conjugate-gradient row solves (wals_cg.hip): slots slot_begin .. slot_begin + nslots of the
// side's order, kCgRows rows per workgroup, `steps` CG steps from each row's current value in X.
// A row stopped on p·A·p ≤ 0 gets status 1 and keeps its last iterate.
constexpr int kCgRows = 16;
constexpr int kCgMaxNT = 16;  // k ≤ 256
template <typename T>
struct CgArgs {
  const int32_t* col;     // indexed with desc.beg (the global rowptr's offsets)
  const T* val;
  const T* Y;             // fixed side [nY][kp]
  const T* G;             // YᵀY of the fixed side, kp×kp
  T* X;                   // solved side [nX][kp]: in x₀, out x
  double* rowloss;
  int32_t* status;        // zero on entry
  const RowDesc* desc;    // slot → CSR range and row
  int64_t slot_begin, nslots;
  T alpha, lambda;
  int steps;
};
hipError_t launch_wals_cg(const CgArgs<float>& a, int nt, hipStream_t s);
hipError_t launch_wals_cg(const CgArgs<double>& a, int nt, hipStream_t s);

// out[0] = *loss, out[1..2] = fb[0..1], out[3] = *chol (0 when chol is null)
hipError_t launch_half_status(const double* loss, const unsigned long long* fb,
                              const int32_t* chol, double* out, hipStream_t s);

// BPR (bpr.hip)
template <typename T>
struct BprArgs {
  T* U;                    // [nu][KP]
  T* I;                    // [ni][KP]
  T* bias;                 // [ni] or nullptr
  const int64_t* pos_user; // positives in data order
  const int32_t* pos_item;
  int64_t npos;
  const int64_t* urowptr;  // user -> sorted positive items (rejection set)
  const int32_t* uitems;
  int64_t nitems;
  int num_neg;
  uint64_t seed;
  uint64_t perm_a, perm_b; // epoch permutation of positives: idx = (a*i + b) mod npos
  T lr, bias_lambda, user_lambda, item_lambda;
  int use_biases;
  int kp;                  // row stride (padded factors)
  int32_t* bad;            // set to 1 if a derivative was not finite
  int waves;               // concurrent waves of the epoch kernel (Hogwild width)
  int atomic_user;         // 1: add the user row's net change atomically (heavy users)
  int capped;              // 1: some user holds ≥ 98% of the items, a draw can end at the
                           // attempt cap with a positive (host-only: picks the kernel)
};

hipError_t launch_bpr_epoch(const BprArgs<float>& a, int kp, hipStream_t s);
hipError_t launch_bpr_epoch(const BprArgs<double>& a, int kp, hipStream_t s);
hipError_t launch_bpr_apply(const BprArgs<float>& a, const int64_t* trip, int64_t n,
                            int kp, hipStream_t s);
hipError_t launch_bpr_apply(const BprArgs<double>& a, const int64_t* trip, int64_t n,
                            int kp, hipStream_t s);
hipError_t launch_bpr_eval(const float* U, const float* I, const float* bias,
                           const int64_t* trip, int64_t n, int kp, int use_biases,
                           double* partial, double* out, hipStream_t s);
hipError_t launch_bpr_eval(const double* U, const double* I, const double* bias,
                           const int64_t* trip, int64_t n, int kp, int use_biases,
                           double* partial, double* out, hipStream_t s);

// BPR fold-in (bpr_foldin.hip): SGD on new users' rows alone, items and biases frozen.  One
// wave64 per row; row r starts from X[r] and ends there, its positives are col[rowptr[r]] ..
// col[rowptr[r + 1]] (strictly ascending).
template <typename T>
struct BprFoldArgs {
  const T* I;              // [ni][KP]
  const T* bias;           // [ni], nullptr: no biases
  const int64_t* rowptr;   // [nrows + 1]
  const int32_t* col;
  T* X;                    // [nrows][KP] in: start values, out: the folded rows
  double* losses;          // [nrows] Σ log(1 + exp(−x̂)) over the last pass's steps
  const T* lr;             // [nepochs] learning rate of every pass
  int64_t nrows;
  int64_t nitems;
  int nepochs, num_neg;
  uint64_t seed;
  T user_lambda;
  int kp;
  int32_t* bad;            // set to 1 if a derivative was not finite
  int grid;                // workgroups (waves); rows past it are reached by striding
};
// the launch's grid for nrows rows (QMFX_BPR_FOLD_GRID lowers it for the tests)
int bpr_fold_grid(int64_t nrows);
hipError_t launch_bpr_fold(const BprFoldArgs<float>& a, hipStream_t s);
hipError_t launch_bpr_fold(const BprFoldArgs<double>& a, hipStream_t s);

// Synthetic data + CSR build (data.hip)
hipError_t launch_synth_keys(uint64_t* keys, int64_t n, uint64_t space, uint64_t seed,
                             hipStream_t s);
// uniform user, Zipf(zipf_s) item popularity (keys u·nitems + i, duplicates possible)
hipError_t launch_synth_keys_zipf(uint64_t* keys, int64_t n, uint64_t nusers, uint64_t nitems,
                                  double zipf_s, uint64_t seed, hipStream_t s);
hipError_t build_csr_from_sorted_keys(const uint64_t* keys, int64_t nnz, int64_t nrows,
                                      uint64_t ncols, int64_t* rowptr, int32_t* col,
                                      hipStream_t s);
hipError_t launch_transpose_keys(const uint64_t* keys, int64_t nnz, uint64_t ncols,
                                 uint64_t nrows, uint64_t* out, hipStream_t s);
hipError_t launch_synth_values_any(const uint64_t* keys, int64_t n, uint64_t div,
                                   uint64_t nitems, int user_major, uint64_t seed, void* val,
                                   int prec, hipStream_t s);
hipError_t sort_unique_keys(uint64_t* keys, uint64_t* scratch, int64_t n, int64_t* n_out,
                            int end_bit, hipStream_t s);
hipError_t sort_keys(uint64_t* keys, uint64_t* scratch, int64_t n, int end_bit, hipStream_t s);
// Device ingest (ingest.hip): packed 24-byte (user id, item id, value) records already on
// the device → ascending id tables and both CSR orientations (buffers allocated by the
// callee, owned by the caller; val in the context precision).
struct IngestOut {
  int64_t n[2] = {0, 0};   // distinct users, items
  DevPtr<int64_t> ids[2];  // ascending ids
  DevPtr<int64_t> rowptr[2];
  DevPtr<int32_t> col[2];
  DevPtr<void> val[2];
};
hipError_t group_records(const void* d_records, int64_t n, int prec, IngestOut& out,
                         hipStream_t s);

hipError_t launch_fill_uniform(float* X, int64_t n, int kp, int k, double bound,
                               uint64_t seed, hipStream_t s);
hipError_t launch_fill_uniform(double* X, int64_t n, int kp, int k, double bound,
                               uint64_t seed, hipStream_t s);

// Test-set ranking statistics (eval.hip)
template <typename T>
struct EvalArgs {
  const T* U;               // [nu][kp]
  const T* I;               // [ni][kp]
  const T* bias;            // [ni] item biases or nullptr
  const int64_t* users;     // [ntest] test user rows
  int64_t ntest;
  int64_t nitems;
  int k, kp;
  // labelled (user, item) pairs, grouped by test slot
  const int32_t* lab_slot;  // [nlab]
  const int64_t* lab_item;  // [nlab]
  const int64_t* lab_pidx;  // [nlab] index into the positives, or -1 (label <= 0)
  int64_t nlab;
  double* lab_score;        // [nlab] out
  // positives (label > 0), grouped by test slot: pptr[t]..pptr[t+1]
  const int64_t* pptr;      // [ntest + 1]
  double* pscore;           // [npos] scores (written by the label pass)
  unsigned long long* above;  // [npos] items scored strictly higher (zeroed by the caller)
  double* sq_part;          // [eval_chunks(ntest, nitems)][ntest] Σ score² per item chunk
  double* udbl;             // [eval_user_rows(ntest)][k] scratch: one batch's test users' rows
  int64_t chunk;            // set by the launcher
  int64_t t_base;           // set by the launcher: first test user of the current batch
};
int64_t eval_chunks(int64_t ntest, int64_t nitems);
int64_t eval_user_rows(int64_t ntest);
int64_t eval_batch_groups();
hipError_t launch_eval_ranks(const EvalArgs<float>& a, hipStream_t s);
hipError_t launch_eval_ranks(const EvalArgs<double>& a, hipStream_t s);

// Top-N recommendations (recommend.hip)
constexpr int kRecMaxN = 128;  // QMFX_REC_MAX_N
template <typename T>
struct RecArgs {
  const T* U;                // [nu][kp]
  const T* I;                // [ni][kp]
  const T* bias;             // [ni] item biases or nullptr
  const int64_t* users;      // [nreq] requested user rows (any order, repeats allowed)
  int64_t nreq;
  int64_t nitems;
  int k, kp;
  int topn;                  // 1..kRecMaxN
  // the users' seen items, ascending within a user: row r is seen_col[seen_ptr[r]] ..
  // seen_col[seen_ptr[r + 1]]; seen_ptr = nullptr: every item is eligible
  const int64_t* seen_ptr;
  const int32_t* seen_col;
  double* udbl;              // [eval_user_rows(nreq)][k] scratch: one batch's users' rows
  // per-chunk survivors of one batch, [eval_chunks(nreq, nitems)][eval_user_rows(nreq)] lists
  double* part_score;        // [lists][topn]
  int32_t* part_item;        // [lists][topn]
  int32_t* part_cnt;         // [lists]
  int64_t* items;            // [nreq][topn] out: item rows in rank order, −1 in the unused tail
  double* scores;            // [nreq][topn] out: their scores, 0.0 in the unused tail
  int32_t* counts;           // [nreq] out: min(topn, eligible items)
  int64_t chunk;             // set by the launcher
  int64_t t_base, nbatch;    // set by the launcher: first user and user rows of the batch
  // deny list (qmfx_recommend_without): bit i % 64 of word i / 64 set = item i is eligible for
  // nobody; nullptr: none.  Only launch_recommend reads it.
  const unsigned long long* deny;  // [(nitems + 63) / 64]
};
hipError_t launch_recommend(const RecArgs<float>& a, hipStream_t s);
hipError_t launch_recommend(const RecArgs<double>& a, hipStream_t s);

// Top-N within candidate lists (recommend.hip, qmfx_recommend_candidates): the selection of
// RecArgs over listed items only.  cptr == nullptr: every user ranks the shared list
// cand[0 .. ncand); else user t ranks cand[cptr[t] .. cptr[t + 1]).  A list is strictly
// ascending.  A list of n candidates is cut into cand_chunks(n) chunks; the per-user form runs
// one wave per work item (user, chunk): user t owns the work items woff[t] .. woff[t + 1], and
// wuser maps a work item back to its user.  Partial lists: shared form
// [cand_chunks(ncand)][eval_user_rows(nreq)], per-user form one per work item (woff[nreq]).
int64_t cand_chunks(int64_t n);
template <typename T>
struct CandArgs : RecArgs<T> {
  const int32_t* cand;       // the lists' item rows
  int64_t ncand;             // shared form: the list's length
  const int64_t* cptr;       // [nreq + 1] or nullptr
  const int64_t* woff;       // [nreq + 1] per-user form: first work item of every user
  const int32_t* wuser;      // [woff[nreq]] per-user form: the user (position in users) of an item
  const int64_t* h_woff;     // woff on the host (the launcher batches by it)
  int64_t w_base, w_end;     // set by the launcher: the batch's work items
};
hipError_t launch_recommend_candidates(const CandArgs<float>& a, hipStream_t s);
hipError_t launch_recommend_candidates(const CandArgs<double>& a, hipStream_t s);

// Top-N neighbours of a side's rows among the rows of the same side (recommend.hip): the
// selection of RecArgs with U = I = the side's factors, users = the query rows, nitems = the
// side's rows, no bias and no seen lists.
template <typename T>
struct SimArgs : RecArgs<T> {
  const double* norms;       // [nitems] row norms (launch_factor_norms); cosine only
  int cosine;                // 0: dot, else dot / (norm · norm)
  int exclude_self;          // the query row itself is not eligible
};
hipError_t launch_similar(const SimArgs<float>& a, hipStream_t s);
hipError_t launch_similar(const SimArgs<double>& a, hipStream_t s);
// norms[r] = sqrt(Σ_f F[r][f]²) in double, the sum in factor order with one rounded multiply
// and one rounded add per factor
hipError_t launch_factor_norms(const float* F, int64_t n, int k, int kp, double* norms,
                               hipStream_t s);
hipError_t launch_factor_norms(const double* F, int64_t n, int k, int kp, double* norms,
                               hipStream_t s);

// The screen of qmfx_recommend_screened (screen.hip): an f32 MFMA scan of request × catalogue
// that appends to user t's list every item the bound of include/qmfx.h cannot rule out of the
// user's top-N.  T is the context precision (the type of the biases).
constexpr int kScreenTileUsers = 128, kScreenTileItems = 128;  // a workgroup's tile
template <typename T>
struct ScreenArgs {
  const float* A;            // [nreq][kp] the requested users' rows, rounded to f32
  const float* B;            // [nitems][kp] the items' rows, rounded to f32
  const T* bias;             // [nitems] item biases or nullptr
  int64_t nreq, nitems;
  int k, kp;
  const double* unorm;       // [nreq] norms of the requested rows (launch_factor_norms)
  const double* inorm;       // [nitems]
  const double* thr;         // [nreq] L_u; +inf: nothing finite passes
  int32_t* cnt;              // [nreq] passing items, zero on entry; runs past cap
  int32_t* list;             // [nreq][cap] the first cap passing items, in no order
  int64_t cap;
  int64_t itiles;            // set by the launcher: item tiles
};
// workgroups of a scan (one grid dimension); a launch's thread count must fit 32 bits, so a scan
// of more than kScreenMaxTiles is refused
constexpr int64_t kScreenMaxTiles = ((int64_t)1 << 31) / 256 - 1;
int64_t screen_tiles(int64_t nreq, int64_t nitems);
hipError_t launch_screen(const ScreenArgs<float>& a, hipStream_t s);
hipError_t launch_screen(const ScreenArgs<double>& a, hipStream_t s);
// out[t][·] = U[users[t]][·] (all kp columns)
hipError_t launch_screen_gather(const float* U, const int64_t* users, int64_t nreq, int kp,
                                float* out, hipStream_t s);
hipError_t launch_screen_gather(const double* U, const int64_t* users, int64_t nreq, int kp,
                                double* out, hipStream_t s);
hipError_t launch_screen_f32(const double* in, int64_t n, float* out, hipStream_t s);
// thr[t] = scores[t][topn − 1] when counts[t] == topn, else +inf; cnt[t] = 0; scnt[t] = counts[t]
hipError_t launch_screen_prep(const double* scores, const int32_t* counts, int64_t nreq, int topn,
                              double* thr, int32_t* cnt, int32_t* scnt, hipStream_t s);
// keys[cptr[t] + j] = t << 32 | list[t][j], j < cptr[t + 1] − cptr[t]; and the items back out
hipError_t launch_screen_keys(const int32_t* list, const int64_t* cptr, int64_t nreq, int64_t cap,
                              uint64_t* keys, hipStream_t s);
hipError_t launch_screen_unpack(const uint64_t* keys, int64_t n, int32_t* cand, hipStream_t s);

// Fold-in (foldin.hip): the row plan of a foreign CSR, built on the device.
// A row's sort key, low bits first: [row : row_bits][field : n_bits][direct : 1].  Whitened
// rows (bucket NTN = (max(n, 1) + 15) / 16 ≤ max_ntn) carry field = NTN − 1, direct rows
// field = max_n − n, so one ascending sort yields the buckets in order with rows ascending
// inside, then the direct rows by descending n with ties by ascending row: build_buckets'
// layout for one piece without split-K rows.
struct FoldKeyBits {
  int row_bits, n_bits;
  int end_bit() const { return row_bits + n_bits + 1; }
};
FoldKeyBits fold_key_bits(int64_t nrows, int64_t max_n);
hipError_t launch_fold_keys(const int64_t* rowptr, int64_t nrows, int max_ntn, int64_t max_n,
                            FoldKeyBits kb, uint64_t* keys, hipStream_t s);
// sorted keys → order[nrows], desc[nrows] and wb[kMaxNTN + 1]: the first slot of every
// whitened bucket, wb[kMaxNTN] = the first direct slot
hipError_t launch_fold_expand(const uint64_t* keys, const int64_t* rowptr, int64_t nrows,
                              FoldKeyBits kb, int64_t* order, RowDesc* desc, int64_t* wb,
                              hipStream_t s);
// out[r·k + f] = X[r·kp + f] widened (the solved rows without their padding columns)
hipError_t launch_fold_gather(const float* X, int64_t nrows, int k, int kp, double* out,
                              hipStream_t s);
hipError_t launch_fold_gather(const double* X, int64_t nrows, int k, int kp, double* out,
                              hipStream_t s);
hipError_t launch_iota(int64_t* out, int64_t n, hipStream_t s);  // out[i] = i

// Explanations (explain.hip): per-signal contributions c_e·y_eᵀA⁻¹y_t to a row's score of a
// target, from one kept Cholesky factor of the row's system per query.
constexpr int kExplainRhs = 8;          // right-hand sides (targets) solved together
constexpr int kExplainLdsMaxKP = 128;   // the packed factor lives in LDS up to this KP
template <typename T>
struct ExplainArgs {
  // of sys: col, val (indexed with rowptr's offsets), Y, G, alpha, lambda, k, kp; scratch: one
  // packed triangle KP(KP+1)/2 per workgroup when KP > kExplainLdsMaxKP
  FallbackArgs<T> sys;
  const int64_t* rowptr;   // CSR of the explained rows
  const int64_t* rows;     // [nq] row of query q, or nullptr: query q is row q
  int64_t nq;
  const int64_t* qptr;     // [nq + 1] query q explains targets[qptr[q] .. qptr[q + 1])
  const int64_t* targets;  // row indices of Y
  int topm;                // 1..kRecMaxN
  int64_t* sources;        // [npairs][topm] column of the signal, −1 in the unused tail
  int64_t* positions;      // [npairs][topm] its position in the row, −1 in the tail
  double* contribs;        // [npairs][topm] 0.0 in the tail
  int32_t* counts;         // [npairs] min(topm, n)
  double* totals;          // [npairs]
  double* all;             // nullptr, or every contribution: query q's pairs from allq[q], n each
  const int64_t* allq;     // [nq]
  unsigned long long* first_bad;  // the smallest query whose system is not positive definite
};
int explain_grid(int64_t nq, int kp);
hipError_t launch_explain(const ExplainArgs<float>& a, hipStream_t s);
hipError_t launch_explain(const ExplainArgs<double>& a, hipStream_t s);

}  // namespace qmfx
