/*
 * qmfx.h: C ABI of the MI355X (gfx950) implicit-feedback MF engine.
 *
 * This is the device layer under the drop-in qmf::Engine API (qmf_amd/host/qmf/).  It
 * replaces the reference's in-process CPU hot path (taozhijiang/qmf, paths relative to the
 * reference root):
 *
 *   qmf/wals/WALSEngine.cpp:165-218  WALSEngine::iterate           -> qmfx_wals_half
 *   qmf/wals/WALSEngine.cpp:246-264  WALSEngine::computeXtX        -> inside qmfx_wals_half
 *   qmf/wals/WALSEngine.cpp:266-310  WALSEngine::updateFactorsForOne -> inside qmfx_wals_half
 *   qmf/Matrix.cpp:81-96             linearSymmetricSolve (dsysv_) -> inside qmfx_wals_half
 *   qmf/wals/WALSEngine.cpp:130-163  groupSignals / sortDataset    -> qmfx_group_signals (device
 *   qmf/utils/IdIndex.cpp:21-31      IdIndex (id -> idx)              sort + CSR build), qmfx_get_ids;
 *                                                                     qmfx_upload_csr / qmfx_gen_synthetic
 *   qmf/FactorData.h:55-100          FactorData::setFactors        -> qmfx_set_factors / qmfx_fill_uniform
 *   qmf/bpr/BPREngine.cpp:146-220    BPREngine::optimize / update  -> qmfx_bpr_epoch / qmfx_bpr_apply
 *   qmf/bpr/BPREngine.cpp:246-274    BPREngine::evaluate (loss)    -> qmfx_bpr_eval
 *   distributed/ (TCP broadcast + bucket gather)                   -> qmfx_dist_init + qmfx_wals_half
 *                                                                     (RCCL all-gather over xGMI)
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Host buffers are copied;
 * device buffers are owned by the context.  Every call returns 0 on success or a negative
 * code, with a message from qmfx_last_error() (thread-local).  The reference aborts on
 * errors (glog CHECK); the C++ wrapper converts a non-zero status into that abort.  One
 * caller thread per context.  Sides: 0 = users, 1 = items.  Factors cross the ABI as
 * row-major float64 n×k (the reference's Double = double, qmf/Types.h:24); on the device
 * they are stored in the context precision (32 or 64) with rows padded to a multiple of 16.
 */
#ifndef QMFX_H_
#define QMFX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qmfx_ctx qmfx_ctx;

#define QMFX_USERS 0
#define QMFX_ITEMS 1

/* ---- library / context ---------------------------------------------------------------- */
const char* qmfx_last_error(void);
int qmfx_version(void);
int qmfx_device_count(int* count);

/* precision: 32 or 64.  nfactors: the reference's --nfactors (WALSConfig/BPRConfig). */
int qmfx_create(qmfx_ctx** out, int device, int precision, int nfactors);
int qmfx_destroy(qmfx_ctx* ctx);
int qmfx_sync(qmfx_ctx* ctx);
/* A changed row count releases what the old one sized or indexed: that side's factors and
   CSR; with either side, the test labels, the BPR positives and the cached qmfx_bpr_eval
   triplets; with the item count, the item biases.  The same shape again keeps all of these. */
int qmfx_set_shape(qmfx_ctx* ctx, int64_t nusers, int64_t nitems);
int qmfx_get_shape(qmfx_ctx* ctx, int64_t* nusers, int64_t* nitems, int64_t* nnz);

/* ---- interactions (WALSEngine.cpp:130-163) --------------------------------------------- */
/* CSR of `side`: rowptr[n_side+1], colidx[nnz] = row index on the other side, values[nnz]. */
int qmfx_upload_csr(qmfx_ctx* ctx, int side, const int64_t* rowptr, const int32_t* colidx,
                    const double* values, int64_t nnz);
/* Device ingest of raw interactions (WALSEngine::init / groupSignals / sortDataset,
 * WALSEngine.cpp:37-69, 130-163; IdIndex.cpp:21-31).  `records` holds nnz packed 24-byte
 * records in the reference's DatasetElem layout (DatasetReader.h:29-33: int64 userId,
 * int64 itemId, double value), in file order.  Sets the shape (distinct users, items) and
 * builds both CSR orientations on the device: rows in ascending-id order, entries by
 * ascending column id, duplicate (u, i) pairs kept in input order.  nnz < 2^31. */
int qmfx_group_signals(qmfx_ctx* ctx, const void* records, int64_t nnz, int64_t* nusers,
                       int64_t* nitems);
/* Ascending distinct ids of `side` (n_side values; idx = position), after
 * qmfx_group_signals. */
int qmfx_get_ids(qmfx_ctx* ctx, int side, int64_t* ids);
/* Device-generated synthetic matrix: ~nnz uniform unique (u, i) pairs,
 * w in 1..5, both orientations built on the device.  *nnz_out = unique pairs kept. */
int qmfx_gen_synthetic(qmfx_ctx* ctx, int64_t nusers, int64_t nitems, int64_t nnz,
                       uint64_t seed, int64_t* nnz_out);
/* Skewed variant (SURVEY.md §8(d) "Zipf(s=1.0) item popularity", power-law rows): `ndraws`
 * (user uniform, item rank ~ continuous Zipf(zipf_s)) draws, duplicates dropped; zipf_s = 0
 * is qmfx_gen_synthetic.  *nnz_out = unique pairs kept. */
int qmfx_gen_synthetic_zipf(qmfx_ctx* ctx, int64_t nusers, int64_t nitems, int64_t ndraws,
                            uint64_t seed, double zipf_s, int64_t* nnz_out);
/* dst takes src's interactions (shape, id tables and both CSR orientations, copied device to
 * device: over xGMI between GPUs) instead of building them again: one qmfx_group_signals for
 * an n-GPU engine, then an import per peer before qmfx_dist_init_all shards them.  Both
 * contexts must have the same precision; src must not be sharded and dst must not have been
 * through qmfx_dist_init[_all].  src's stream is synchronised before the copies. */
int qmfx_import_signals(qmfx_ctx* dst, qmfx_ctx* src);
/* Copies a side's CSR back to the host (e.g. for CPU baselines on the same data).  values are
 * returned in double, exactly as the device holds them (an fp32 context's values widened). */
int qmfx_download_csr(qmfx_ctx* ctx, int side, int64_t* rowptr, int32_t* colidx,
                      double* values);

/* ---- factors (FactorData.h) ------------------------------------------------------------- */
int qmfx_set_factors(qmfx_ctx* ctx, int side, const double* rowmajor);
int qmfx_get_factors(qmfx_ctx* ctx, int side, double* rowmajor);
int qmfx_fill_uniform(qmfx_ctx* ctx, int side, double bound, uint64_t seed);

/* ---- WALS (WALSEngine.cpp:165-218) -------------------------------------------------------
 * Solves every row of `side` with the other side fixed: X ← 0, G = YᵀY, per row
 * A = G + Σ αv yyᵀ + λI, b = Σ (1+αv) y, x = A⁻¹b.  *loss_sum receives Σ over solved rows of
 * Σ(1+αv) + xᵀ(A−λI)x − 2xᵀb (divide by nusers·nitems for the reference's printed loss).
 * With a distributed context the local row range is solved and the factor matrix is
 * all-gathered over RCCL before returning; the loss is then the global sum. */
int qmfx_wals_half(qmfx_ctx* ctx, int side, double alpha, double lambda, double* loss_sum);
/* The same half by conjugate gradients (opt-in; one device): every row r of `side` with n ≥ 1
 * signals (column j_e, value v_e; w_e = α·v_e, c_e = 1 + α·v_e, y_j = row j of the other side
 * as the device holds it) takes `steps` CG steps on A·x = b from its current value,
 *   A·v = G·v + Σ_e w_e·(y_{j_e}·v)·y_{j_e} + λ·v  (G = YᵀY; A is never formed),  b = Σ_e c_e·y_{j_e}.
 * Start: x₀ = the row as the context holds it (X is not zeroed; a side never set is all zeros),
 * r = b − A·x₀, p = r, ρ = r·r.  Step t = 0 .. steps−1: stop if ρ == 0; q = A·p, d = p·q; if
 * !(d > 0) (NaN included) the row is flagged and stops with its last iterate; a = ρ/d,
 * x += a·p, r −= a·q, ρ′ = r·r, p = r + (ρ′/ρ)·p, ρ = ρ′.  x is stored in the context
 * precision.  The row's term of *loss_sum is Σc_e + xᵀ(A−λI)x − 2xᵀb on the stored iterate with
 * A·x = b − r, written where qmfx_wals_row_losses reads it.  A row without signals is exactly 0
 * with loss 0.  A flagged row (possible only when some 1 + α·v < 0 or λ ≤ 0) is listed by
 * qmfx_wals_failed_rows; there is no pivoted re-solve for it.  fp64 contexts compute in double;
 * fp32 contexts keep the vectors in f32 and accumulate ρ, d and the loss in double.
 * Rows of the split-K heavy class ([9] of qmfx_row_classes) are solved exactly, as
 * qmfx_wals_half solves them: they are few, and one wave must not serialise a million gathers
 * per step.
 * Fails with -1 before anything is launched when side is not 0 or 1, steps < 1, `side` has no
 * CSR, the other side has no factors, nfactors > 256, or the context was sharded by
 * qmfx_dist_init*.  The fixed side, the CSR, the biases and the evaluation state are left as
 * they are.  The device time and (steps+1)·(2k² + 4nk) flop per CG row (the exact formula for a
 * heavy row) go into qmfx_solve_kernel_stats. */
int qmfx_wals_half_cg(qmfx_ctx* ctx, int side, double alpha, double lambda, int steps,
                      double* loss_sum);
/* Number of rows whose system the Cholesky kernels could not factor in the last half (a
 * non-positive pivot: some 1 + α·v < 0, λ ≤ 0, or fp32 rounding on a nearly singular
 * system); their indices go to rows[] (up to cap).  qmfx_wals_half has already re-solved
 * them on the device in fp64 with partial pivoting (dsysv_'s role, Matrix.cpp:81-96) before
 * the half's all-gather, and failed with -6 if one was exactly singular (CHECK(info == 0),
 * Matrix.cpp:94). */
int qmfx_wals_failed_rows(qmfx_ctx* ctx, int64_t* rows, int64_t cap, int64_t* count);
/* The row plan of `side` on this rank (11 counts): [0..7] whitened rows in the n×n buckets
 * n ≤ 16·(i+1) (used when λ > 0), [8] direct k×k rows, [9] split-K heavy rows (more than
 * QMFX_HEAVY_MIN signals, default 16384; every k: the one-wave direct tilings and the multi-wave
 * k > 128 kernel), [10] their
 * segments (QMFX_SEG_LEN signals each, default 8192). */
int qmfx_row_classes(qmfx_ctx* ctx, int side, int64_t* counts);
/* Per-row loss terms of the last half (n_side values; the sum is *loss_sum). */
int qmfx_wals_row_losses(qmfx_ctx* ctx, double* out);
/* One row's system as the reference forms it (updateFactorsForOne, WALSEngine.cpp:266-299),
 * built on the device in fp64 from the current fixed side: A (k×k row-major, λ included),
 * b and Σ(1 + αv). */
int qmfx_wals_row_system(qmfx_ctx* ctx, int side, int64_t row, double alpha, double lambda,
                         double* A, double* b, double* csum);
int qmfx_wals_set_row(qmfx_ctx* ctx, int side, int64_t row, const double* x);

/* ---- BPR (BPREngine.cpp:146-274) ---------------------------------------------------------
 * Positives in data order as (user idx, item idx) (BPREngine::init :65-82).  Builds the
 * per-user sorted positive lists used for negative rejection. */
int qmfx_bpr_set_positives(qmfx_ctx* ctx, const int64_t* users, const int64_t* items,
                           int64_t npos);
int qmfx_bpr_set_biases(qmfx_ctx* ctx, const double* bias);  /* nitems values */
int qmfx_bpr_get_biases(qmfx_ctx* ctx, double* bias);
/* One Hogwild epoch over all positives × num_neg sampled negatives, visiting positives in
 * a seed-dependent permuted order when shuffle != 0. */
int qmfx_bpr_epoch(qmfx_ctx* ctx, uint64_t seed, int num_neg, double lr, double bias_lambda,
                   double user_lambda, double item_lambda, int use_biases, int shuffle);
/* Applies the given (u, p, n) triplets in order with one wave (exact update order). */
int qmfx_bpr_apply(qmfx_ctx* ctx, const int64_t* triplets, int64_t n, double lr,
                   double bias_lambda, double user_lambda, double item_lambda, int use_biases);
/* Σ log(1+exp(−x̂)) over triplets (host array, uploaded and cached per `slot` 0/1).  The
 * cache is keyed by the array's host address and length: another array or length is uploaded
 * again, an array rewritten in place at the same length is not. */
int qmfx_bpr_eval(qmfx_ctx* ctx, int slot, const int64_t* triplets, int64_t n, int use_biases,
                  double* loss_sum);

/* ---- test-set evaluation (Engine::computeTestScores Engine.cpp:73-96 + Metrics.cpp:27-164)
 * The device replaces the dense n_test × n_items score matrix by the statistics every
 * reference metric (mse, auc, ap, p@k, r@k) is a function of.
 * qmfx_eval_set_labels: test users (user idx, ntest of them) and their labelled items as a
 * CSR over the test slots (rowptr[ntest+1], item idx, label value; zero labels may be left
 * out).  Labels > 0 are the positives.  Cached on the context until the next call. */
int qmfx_eval_set_labels(qmfx_ctx* ctx, int64_t ntest, const int64_t* users,
                         const int64_t* rowptr, const int64_t* items, const double* values);
/* Scores the current factors (score = [bias_i +] <u, q_i>, the reference's double, bit for
 * bit; use_biases adds the context's item biases) and returns
 *   label_scores[rowptr[ntest]]  the score of every labelled pair, in CSR order;
 *   above[npos]                  per positive (labelled pair with value > 0, in CSR order):
 *                                the number of items scored strictly higher;
 *   sq_sum[ntest]                Σ over all items of score². */
int qmfx_eval_ranks(qmfx_ctx* ctx, int use_biases, double* label_scores, int64_t* above,
                    double* sq_sum);

/* ---- top-N recommendations -------------------------------------------------------------------
 * For each of the nusers requested users (user idx; any order, repeats allowed) the device
 * scores every item and selects the user's best eligible items, without the dense score
 * matrix.  score(u, i) is exactly qmfx_eval_ranks' score: the item bias when use_biases (else
 * 0.0), then s = s + u_f * q_f for f = 0..k-1 in double, one rounded multiply and one rounded
 * add each, on the factor values the device holds (an fp32 context's values widened).
 * Item a ranks before item b when score_a > score_b, or score_a == score_b and a < b: the
 * comparison is numeric (-0.0 equals +0.0, then the index decides).  NaN scores are out of
 * contract: the order is undefined then.
 * Eligible items, by `exclude`: every item (QMFX_REC_ALL), or every item not in the user's
 * seen list: the user's row of the side-0 CSR (QMFX_REC_UNSEEN_SIGNALS; needs the column
 * indices ascending within a row, which qmfx_group_signals and the synthetic generators
 * guarantee and which is the caller's precondition for qmfx_upload_csr), or the user's
 * qmfx_bpr_set_positives items (QMFX_REC_UNSEEN_POSITIVES).
 * User t's recommendation is the first counts[t] = min(topn, eligible) eligible items in that
 * order: items[t*topn + r] (item idx) and scores[t*topn + r] for rank r; the unused tail
 * carries item -1 and score 0.0.  topn is 1..QMFX_REC_MAX_N.
 * Fails (-1, with a message) on: topn out of range, a user index out of range, an exclude
 * mode whose data is absent, use_biases without biases, nfactors > 256, no factors.  On a
 * context sharded by qmfx_dist_init* QMFX_REC_UNSEEN_SIGNALS accepts only users of this
 * rank's row range (it holds no other rows' signals); the other two modes work on any rank,
 * the factors being full replicas.  nusers == 0 succeeds and touches nothing. */
#define QMFX_REC_MAX_N 128
#define QMFX_REC_ALL 0              /* every item is eligible */
#define QMFX_REC_UNSEEN_SIGNALS 1   /* minus the user's row of the side-0 CSR (WALS) */
#define QMFX_REC_UNSEEN_POSITIVES 2 /* minus the user's qmfx_bpr_set_positives list (BPR) */
int qmfx_recommend(qmfx_ctx* ctx, int64_t nusers, const int64_t* users, int topn, int exclude,
                   int use_biases, int64_t* items /*nusers·topn*/, double* scores /*nusers·topn*/,
                   int32_t* counts /*nusers*/);

/* ---- recommendations within candidate sets -----------------------------------------------------
 * qmfx_recommend with fewer eligible items.  Scores (bit for bit), order and tie rule, counts[t] =
 * min(topn, eligible), the -1 / 0.0 tail, the three exclude modes (the own-rows rule of
 * QMFX_REC_UNSEEN_SIGNALS on a sharded context included) and use_biases are qmfx_recommend's.
 * qmfx_recommend_without: the ndeny items of `deny` (item idx; any order, repeats allowed) are
 * eligible for nobody, on top of `exclude`.  The whole catalogue is still scanned: one bit per
 * item is uploaded and the selection skips the set ones.  ndeny == 0 is qmfx_recommend.
 * qmfx_recommend_candidates: only listed items are eligible, and only they are scored (their
 * rows are gathered by index: the work follows the lists' lengths, not the catalogue's).
 * cptr == NULL: one list cand[0 .. ncand) shared by all requested users; cptr != NULL: user t's
 * list is cand[cptr[t] .. cptr[t+1]) and ncand is ignored (a repeated user may carry different
 * lists).  Every list is strictly ascending item idx; an empty list gives count 0.  A shared
 * list of every item is qmfx_recommend exactly.  A deny list and candidate lists do not combine
 * in one call: the caller removes denied items from its lists.
 * Fail (-1, with a message, before anything is launched) on everything qmfx_recommend rejects
 * and on: ndeny < 0 or ncand < 0, a deny or candidate index out of range, cptr[0] != 0 or cptr
 * decreasing, a list that is not strictly ascending, 2^31 candidates or more in total.
 * nusers == 0 succeeds and touches nothing.  The calls leave the factors, CSR, biases and every
 * cached state untouched; their scratch is sized from the request and owned by the context.
 * Their kernel time is counted in qmfx_solve_kernel_stats with 2k flop per (user, item scanned)
 * pair for the deny call and 2k flop per (user, candidate) pair for the candidate call. */
int qmfx_recommend_without(qmfx_ctx* ctx, int64_t nusers, const int64_t* users, int64_t ndeny,
                           const int64_t* deny, int topn, int exclude, int use_biases,
                           int64_t* items /*nusers·topn*/, double* scores /*nusers·topn*/,
                           int32_t* counts /*nusers*/);
int qmfx_recommend_candidates(qmfx_ctx* ctx, int64_t nusers, const int64_t* users,
                              const int64_t* cptr /*NULL or nusers+1*/, int64_t ncand,
                              const int64_t* cand, int topn, int exclude, int use_biases,
                              int64_t* items /*nusers·topn*/, double* scores /*nusers·topn*/,
                              int32_t* counts /*nusers*/);

/* ---- screened recommendations: an f32 filter, an exact re-rank, identical lists ----------------
 * qmfx_recommend_screened returns items, scores and counts of qmfx_recommend for the same
 * arguments, bit for bit (tie rule, -1 / 0.0 tail, the three exclude modes, the own-rows rule of
 * QMFX_REC_UNSEEN_SIGNALS on a sharded context, use_biases), for every input qmfx_recommend
 * accepts; `sample` and `cap` only move work between the stages and never change the answer.
 * It scores the whole catalogue once in f32 on the matrix cores and scores exactly only what the
 * f32 pass cannot rule out:
 *   Sample      the S = `sample` items floor(j * nitems / S), j = 0..S-1.
 *   Threshold   L_u = the score at rank topn-1 of user u's exact top-N within the sample (same
 *               exclude and bias; the shared-list form of qmfx_recommend_candidates).  A user
 *               whose sample holds fewer than topn eligible items is answered by the exact scan
 *               (qmfx_recommend's).
 *   Screen      a(u, i) = the f32 fma chain s = fmaf(u^_f, q^_f, s), f = 0..k-1 from s = 0, of the
 *               rows rounded to f32 (round to nearest even; the identity on an fp32 context).
 *   Slack       eps(u, i) = (k + 4) * 2^-23 * nu * nq  +  (k + 4) * 2^-52 * |b_i|
 *                           +  2^-116 * (1 + nu + nq),
 *               nu and nq the values qmfx_factor_norms returns for the user's and the item's row,
 *               b_i the item's bias (0 without use_biases), evaluated in double.
 *   Pass rule   item i passes for user u unless a is finite and (double)a + b_i < L_u - eps(u, i),
 *               each side one rounded double operation.  A non-finite a always passes.  Seen
 *               items are not looked at here.
 *   Re-rank     a user with at most `cap` passing items is ranked exactly within them (the
 *               per-user form of qmfx_recommend_candidates, lists ascending); a user with more
 *               is answered by the exact scan.
 * Why the lists are identical: every item of the true top-N has an exact score >= the true N-th
 * score >= L_u (the sample is part of the catalogue), |a + b_i - score| <= eps(u, i) whenever a is
 * finite (DESIGN 3.12 derives the constants: one f32 rounding per operand, the f32 chain's
 * gamma_k, Cauchy-Schwarz, the double score's own roundings, and the absolute term for f32
 * underflow with or without subnormals), and rounding is monotone; so it passes, and ranking
 * exactly within a superset of the top-N gives the top-N.
 * sample = 0 / cap = 0 choose them: S = sqrt(8 * topn * nitems) up to a multiple of 64, cap =
 * 4 * topn * nitems / S + 64.  With both 0 a catalogue too small for the screen to pay off is
 * answered by qmfx_recommend's path alone; an explicit sample or cap always screens.
 * Fails (-1, with a message, before anything is launched) on everything qmfx_recommend rejects,
 * on sample not 0 and outside topn..nitems, and on cap not 0 and below topn.  nusers == 0
 * succeeds and touches nothing.  The call leaves the factors, CSR, biases and every cached state
 * untouched; f32 copies and norms are made per call; scratch is sized from the request and owned
 * by the context.  Its device time is counted in qmfx_solve_kernel_stats with 2k flop per (user,
 * item scanned) pair, as qmfx_recommend's is.
 * qmfx_recommend_screen_stats, of the last screened call: [0] users answered through the screen,
 * [1] users answered by the exact scan, [2] candidates kept in total, [3] the longest kept list.
 * qmfx_recommend_screen_stage_ms, of the last screened call: milliseconds on the device stream of
 * [0] sample, [1] rows / norms / f32 copies, [2] screen, [3] counters to the host and sort,
 * [4] re-rank, [5] exact scan (all 0 when the call took the dense path). */
int qmfx_recommend_screened(qmfx_ctx* ctx, int64_t nusers, const int64_t* users, int topn,
                            int exclude, int use_biases, int64_t sample /*0 = auto*/,
                            int64_t cap /*0 = auto*/, int64_t* items /*nusers·topn*/,
                            double* scores /*nusers·topn*/, int32_t* counts /*nusers*/);
int qmfx_recommend_screen_stats(qmfx_ctx* ctx, int64_t out[4]);
int qmfx_recommend_screen_stage_ms(qmfx_ctx* ctx, double out[6]);

/* ---- similar rows: top-N neighbours in factor space ----------------------------------------
 * For each of the nq query rows of `side` (row idx; any order, repeats allowed) the device
 * scores every row of the same side against the query row and selects the best eligible ones,
 * without a score matrix.  All arithmetic is double, on the factor values the device holds (an
 * fp32 context's values widened); item biases are never used.
 *   dot(a, b)     s = 0.0, then s = s + a_f * b_f for f = 0..k-1, one rounded multiply and one
 *                 rounded add each, never fused: qmfx_recommend's score without a bias.
 *   norm(a)       sqrt(dot(a, a)), the sqrt correctly rounded.  qmfx_factor_norms returns
 *                 these values for every row of `side` (n_side doubles).
 *   cosine(a, b)  den = norm(a) * norm(b) (one rounded multiply); dot(a, b) / den (one
 *                 correctly rounded divide) when den > 0, else 0.0: a zero row, or a product
 *                 that underflows to 0, scores 0.0, never NaN.
 * metric selects the score: QMFX_SIM_DOT or QMFX_SIM_COSINE.  The order is qmfx_recommend's:
 * row x ranks before row y when score_x > score_y, or score_x == score_y and x < y; the
 * comparison is numeric (-0.0 equals +0.0).  NaN or infinite factor values are out of contract.
 * Every row of the side is eligible, except, with exclude_self != 0, the row whose index is
 * the query's: exclusion is by index, so an exact duplicate of the query row stays eligible.
 * Query t's answer is the first counts[t] = min(topn, eligible) rows in that order:
 * neighbours[t*topn + r] (row idx) and scores[t*topn + r] for rank r; the unused tail carries
 * -1 and 0.0.  topn is 1..QMFX_REC_MAX_N.
 * Fails (-1, with a message) on: side not 0 or 1, topn out of range, an unknown metric, a row
 * index out of range, no factors, nfactors > 256 (qmfx_similar only).  A context sharded by
 * qmfx_dist_init* answers for any row on any rank, the factors being full replicas.  nq == 0
 * succeeds and touches nothing.  The norms are computed by every call, never cached. */
#define QMFX_SIM_DOT 0
#define QMFX_SIM_COSINE 1
int qmfx_factor_norms(qmfx_ctx* ctx, int side, double* norms /*n_side*/);
int qmfx_similar(qmfx_ctx* ctx, int side, int64_t nq, const int64_t* rows, int topn, int metric,
                 int exclude_self, int64_t* neighbours /*nq·topn*/, double* scores /*nq·topn*/,
                 int32_t* counts /*nq*/);

/* ---- fold-in: rows that were not in the training matrix ------------------------------------
 * qmfx_wals_fold_in solves nrows new rows of `side` against the context's current factors of
 * the other side.  The rows come as a CSR of their own: rowptr[nrows+1], colidx = row idx on
 * the other side, values.  Row r's x is what qmfx_wals_half(side) would write for a row with
 * these signals: the same formulas and row kernels, the context precision, the same pivoted
 * fp64 re-solve of a row the Cholesky kernels flag (*pivoted counts them), and -6 when a row is
 * exactly singular.  factors[r*k + f] carries the values the device holds, widened (an fp32
 * context's rounding is visible, as in qmfx_get_factors); losses[r] is the row's term of a
 * half's *loss_sum.  A row without signals is exactly 0; repeated columns within a row add up,
 * as duplicate pairs do in training.
 * The context needs the shape and the other side's factors only (qmfx_set_shape +
 * qmfx_set_factors): neither a CSR nor factors of `side`.  The call leaves the context's
 * factors, CSR, row buckets and everything qmfx_wals_row_losses / qmfx_wals_failed_rows report
 * about the last half untouched: the new rows, their losses and status words live in scratch
 * of their own, grown on demand.  YᵀY, the whitening of the fixed side and G + λI's image are
 * computed by every call, never cached (they overwrite the buffers every half recomputes).
 * The rows' plan (whitened buckets and direct rows, the limits of qmfx_row_classes;
 * QMFX_NO_WHITEN and QMFX_WB_K64_NTN act as on training) is built on the device; rows of any
 * length are solved whole, never split into segments.  Works on any rank of a sharded context,
 * the factors being full replicas.
 * Fails (-1, with a message, before anything is launched) on: side not 0 or 1, no factors on
 * the fixed side, rowptr[0] != 0 or rowptr decreasing, a column index outside the other side,
 * nrows or rowptr[nrows] >= 2^31.  nrows == 0 succeeds and touches nothing.
 *
 * qmfx_fold_in_classes: the bucket counts of the plan the last fold-in call used, laid out
 * like qmfx_row_classes [0..8]; [9] and [10] are 0.  qmfx_fold_in_order: that plan's
 * processing order (nrows row indices): the whitened buckets in ascending order with rows
 * ascending inside each, then the direct rows by descending signal count, ties by ascending
 * row (what the row buckets of a side hold for the same rows in one piece).
 *
 * qmfx_recommend_fold_in (new users only): folds the rows in as side 0, then selects each new
 * row's top-N as qmfx_recommend defines it: the scores are qmfx_recommend's, bit for bit, on
 * the device-held folded rows and item factors, without biases; the same order and tie rule;
 * the unused tail is -1 / 0.0.  exclude_seen != 0 removes the row's own colidx and needs them
 * ascending within a row (repeats allowed), failing otherwise.  topn is 1..QMFX_REC_MAX_N.
 * factors (NULL or nrows·k) receives the folded rows. */
int qmfx_wals_fold_in(qmfx_ctx* ctx, int side, int64_t nrows, const int64_t* rowptr /*nrows+1*/,
                      const int32_t* colidx, const double* values, double alpha, double lambda,
                      double* factors /*nrows·k*/, double* losses /*nrows or NULL*/,
                      int64_t* pivoted /*NULL or: rows re-solved with pivoting*/);
int qmfx_fold_in_classes(qmfx_ctx* ctx, int64_t* counts /*11*/);
int qmfx_fold_in_order(qmfx_ctx* ctx, int64_t* order /*nrows of the last call*/);
int qmfx_recommend_fold_in(qmfx_ctx* ctx, int64_t nrows, const int64_t* rowptr,
                           const int32_t* colidx, const double* values, double alpha,
                           double lambda, int topn, int exclude_seen, int64_t* items /*nrows·topn*/,
                           double* scores /*nrows·topn*/, int32_t* counts /*nrows*/,
                           double* factors /*NULL or nrows·k*/);

/* ---- BPR fold-in: new users' rows by SGD, items frozen ------------------------------------------
 * qmfx_bpr_fold_in fits nrows new user rows against the context's current item factors (and item
 * biases with use_biases), which are read and never written: BPREngine::update's user line alone.
 * The rows come as a CSR of their own: rowptr[nrows+1], colidx = the row's positive items (item
 * idx), strictly ascending within a row: c_0 < c_1 < ... < c_{n-1}.  Every row is deterministic:
 * its result depends on its own positives, their position in the call's CSR, the seed, the
 * schedule and the items, not on the launch.
 *   Start     p = init[r*k + f] rounded to the context precision; 0.0 with init == NULL.
 *   Passes    for pass e = 0..nepochs-1, for i = 0..n-1 in CSR order in every pass, for
 *             j = 0..num_neg-1: one step on (p, q_{c_i}, q_{n_ij}) at the rate lr_e, with
 *             lr_0 = lr, lr_{e+1} = lr_e * decay in double (BPREngine::optimize's rule), each
 *             rounded once to the context precision.
 *   Draw      qmfx_bpr_epoch's counter-based sampler, in integer arithmetic:
 *             seed_key = mix64(seed ^ 0xb5ad4eceda1ce2a9),
 *             pkey = mix64(mix64(seed_key ^ e) ^ (rowptr[r] + i)), fk = lo32(pkey) ^ hi32(pkey);
 *             attempt t of draw j is cand = (fmix32(fk + (4099*j + t) * 0x9e3779b9) * nitems) >> 32
 *             (mix64: the splitmix64 finaliser, fmix32: murmur3's).  A draw is accepted when cand
 *             is not among the row's positives, or when t >= 4096: a capped draw is used as drawn,
 *             even when it equals c_i.
 *   Step      x = sum_f p_f * (qp_f - qn_f), plus b_p - b_n with use_biases; eg = 1 / (1 + e^x);
 *             p_f <- p_f + lr_e * (eg * (qp_f - qn_f) - user_lambda * p_f), in the context
 *             precision.  A non-finite eg skips the step and flags the call.
 *   Loss      losses[r] = the sum over the steps of the LAST pass, in step order, of
 *             log(1 + exp(-(double)x)), x the step's value before its update.
 * A row without positives keeps its start value and has loss 0.0.  factors[r*k + f] carries the
 * values the device holds, widened, as qmfx_wals_fold_in's does.
 * qmfx_bpr_recommend_fold_in folds the rows in, then selects each new row's top-N exactly as
 * qmfx_recommend defines it: the scores are qmfx_recommend's, bit for bit, on the device-held
 * folded rows and item factors, with the item bias when use_biases; the same order and tie rule;
 * the unused tail is -1 / 0.0.  exclude_seen != 0 removes the row's own colidx.  topn is
 * 1..QMFX_REC_MAX_N.  factors (NULL or nrows*k) receives the folded rows, bit for bit those of
 * qmfx_bpr_fold_in.
 * The context needs only the shape and the item factors (qmfx_set_shape + qmfx_set_factors), plus
 * the biases when use_biases: no user factors, no positives, no CSR.  The calls leave the factors,
 * biases, positives, cached evaluation triplets and everything the last half or epoch reported
 * untouched; the rows, their losses and the passes' rates live in scratch sized from the request
 * and owned by the context (shared with the other fold-in calls).  Both work on any rank of a
 * sharded context, the factors being full replicas.
 * Fail (-1, with a message, before anything is launched) on: no item factors, use_biases without
 * biases, rowptr[0] != 0 or rowptr decreasing, a column index out of range, a row that is not
 * strictly ascending, nepochs < 1 or num_neg < 1, topn out of range, nfactors > 256, nrows or
 * rowptr[nrows] >= 2^31.  nrows == 0 succeeds and touches nothing.  When a step was flagged the
 * call returns -4 with qmfx_bpr_epoch's message, after the outputs are filled.
 * Their device time is counted in qmfx_solve_kernel_stats with the work steps * 6k flop and
 * steps * 2 * kp * (element size) bytes, steps = nepochs * num_neg * rowptr[nrows] and kp = k
 * rounded up to a multiple of 16; the recommend form adds qmfx_recommend's terms. */
int qmfx_bpr_fold_in(qmfx_ctx* ctx, int64_t nrows, const int64_t* rowptr /*nrows+1*/,
                     const int32_t* colidx /*item idx, strictly ascending per row*/,
                     const double* init /*NULL or nrows·k*/, uint64_t seed, int nepochs,
                     int num_neg, double lr, double decay, double user_lambda, int use_biases,
                     double* factors /*nrows·k*/, double* losses /*NULL or nrows*/);
int qmfx_bpr_recommend_fold_in(qmfx_ctx* ctx, int64_t nrows, const int64_t* rowptr,
                               const int32_t* colidx, const double* init, uint64_t seed,
                               int nepochs, int num_neg, double lr, double decay,
                               double user_lambda, int use_biases, int topn, int exclude_seen,
                               int64_t* items /*nrows·topn*/, double* scores /*nrows·topn*/,
                               int32_t* counts /*nrows*/, double* factors /*NULL or nrows·k*/);

/* ---- explanations: per-signal contributions to a recommendation ------------------------------
 * WALS is the model of Hu, Koren and Volinsky (2008); with A = G + Σ αv·yyᵀ + λI and
 * x = A⁻¹ Σ (1+αv)·y the score of a target t splits over the row's own signals:
 *   y_tᵀx = Σ_e (1+αv_e) · y_tᵀ A⁻¹ y_{j_e}.
 * For row r of `side`, its signals in CSR order e = 0..n-1 (column j_e = row idx on the other
 * side, value v_e), w_e = α·v_e, c_e = 1 + α·v_e, and y_j = row j of the other side's factors
 * as the device holds them, widened to double:
 *   A         = G + Σ_e w_e·y_{j_e}y_{j_e}ᵀ + λI: exactly what qmfx_wals_row_system(side, r, α, λ)
 *               returns, G = YᵀY in the context precision, computed by every call, never cached;
 *   z         = A⁻¹y_t for a target t (row idx on the other side), by a Cholesky factorization of
 *               A that is kept and reused for all targets of the query;
 *   contrib_e = c_e · (y_{j_e}·z);  total = Σ_e contrib_e = y_tᵀA⁻¹b = y_t·x̂, x̂ being the row
 *               qmfx_wals_fold_in returns for these signals.
 * All arithmetic after G is double, in both context precisions.  Repeated columns are separate
 * entries with a contribution each.
 * For a TRAINED row `total` is NOT qmfx_recommend's score: the stored x_u was solved against
 * the other side's factors of before the last half that changed them.  For a folded-in row
 * (qmfx_wals_explain_rows with the signals given to qmfx_recommend_fold_in) total is that
 * score, to rounding.
 * Selection: entry a ranks before entry b when contrib_a > contrib_b, or they are equal and
 * a < b by position in the row; the comparison is numeric, as in qmfx_recommend.  Pair p (the
 * position in targets) gets its first counts[p] = min(topm, n) entries in that order:
 * sources[p*topm + s] (column idx), positions[p*topm + s] (entry position in the row) and
 * contribs[p*topm + s]; the unused tail carries -1, -1 and 0.0.  topm is 1..QMFX_REC_MAX_N.
 * The values in the lists are bit for bit those of `all`, which (when not NULL) receives every
 * contribution in CSR order, pair after pair: Σ_p n(row of p) doubles.  A row without signals
 * has count 0 and total exactly 0.0.
 * Explanations are defined for positive definite systems only: when a query's A has a
 * non-positive or non-finite Cholesky pivot (some 1 + αv < 0, or λ ≤ 0) the call returns -5 with
 * a message naming the first such query and fills no output.
 * qmfx_wals_explain explains rows of the context's own CSR of `side`: query q is row rows[q]
 * with targets[qptr[q] .. qptr[q+1]) (repeats allowed, an empty list is fine).  On a context
 * sharded by qmfx_dist_init* it accepts only rows of this rank's row range (the rule of
 * QMFX_REC_UNSEEN_SIGNALS).  qmfx_wals_explain_rows takes the rows as a CSR of their own
 * (qmfx_wals_fold_in's rowptr / colidx / values, validated alike): query q is row q; it needs
 * no CSR on the context and works on any rank.
 * Fail (-1, with a message, before anything is launched) on: side not 0 or 1, topm out of range,
 * a row or target out of range, qptr[0] != 0 or qptr decreasing, no factors on the other side,
 * no CSR of `side` (first form), nfactors > 256.  nq == 0 or no pairs at all succeeds and
 * touches nothing.  The calls leave the factors, the CSR, the row buckets and what the last
 * half reported untouched.  Their kernel time (YᵀY included) is counted in
 * qmfx_solve_kernel_stats with the work  Σ_queries with targets [n·k(k+1) + k³/3]
 * + Σ_pairs [2k² + 2nk] flop.
 * The device solves kExplainRhs = 8 targets of a query at a time; the factor lives in LDS up to
 * 128 (padded) factors and in a context-owned scratch above.
 * qmfx_row_lengths: the signal counts of rows of the context's CSR (host only; the layout of
 * `all` for the first form). */
int qmfx_wals_explain(qmfx_ctx* ctx, int side, int64_t nq, const int64_t* rows,
                      const int64_t* qptr /*nq+1*/, const int64_t* targets, double alpha,
                      double lambda, int topm, int64_t* sources /*npairs·topm*/,
                      int64_t* positions /*npairs·topm*/, double* contribs /*npairs·topm*/,
                      int32_t* counts /*npairs*/, double* totals /*npairs*/,
                      double* all /*NULL or Σ_p n(row of p)*/);
int qmfx_wals_explain_rows(qmfx_ctx* ctx, int side, int64_t nrows, const int64_t* rowptr,
                           const int32_t* colidx, const double* values, const int64_t* qptr,
                           const int64_t* targets, double alpha, double lambda, int topm,
                           int64_t* sources, int64_t* positions, double* contribs,
                           int32_t* counts, double* totals, double* all);
int qmfx_row_lengths(qmfx_ctx* ctx, int side, int64_t n, const int64_t* rows, int64_t* lengths);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) -------------------------------------- */
int qmfx_rccl_unique_id(uint8_t* id128);
/* Joins the RCCL communicator (id128 from rank 0's qmfx_rccl_unique_id), takes this rank's
 * nnz-balanced row range of both sides, rebuilds the row buckets and keeps only this rank's
 * signals on the device.  id128 = NULL sets up the partition without a communicator: each
 * half then solves only this rank's rows and exchanges nothing (tests of the partition). */
int qmfx_dist_init(qmfx_ctx* ctx, int rank, int world, const uint8_t* id128);
/* One process driving n GPUs (the drop-in C++ engine's --ngpus): ctxs[i] (each on its own
 * device, all with the same data and factors) become ranks 0..n-1 of one RCCL clique
 * (ncclCommInitAll), partitioned and sharded as qmfx_dist_init does.  Fails when two
 * contexts share a device or a device is not visible. */
int qmfx_dist_init_all(qmfx_ctx* const* ctxs, int n);
/* qmfx_wals_half over the n contexts of one qmfx_dist_init_all, from one thread: every
 * context's solves are enqueued piece by piece and each piece's all-gather of all ranks is
 * one RCCL group, overlapping the next piece's solves.  *loss_sum: the global sum. */
int qmfx_wals_half_multi(qmfx_ctx* const* ctxs, int n, int side, double alpha, double lambda,
                         double* loss_sum);
/* nnz-balanced contiguous row range owned by `rank` (host-only helper, no GPU needed). */
int qmfx_partition_rows(const int64_t* rowptr, int64_t nrows, int world, int rank,
                        int64_t* begin, int64_t* end);
/* The all-gather schedule of a half-epoch over `world` ranks with `npieces` solve pieces
 * per rank (host only, no device): pbounds[r·(npieces+1) + j] .. [.. + j + 1] is the row
 * range rank r solves as its piece j and then broadcasts to every rank (an empty range is
 * skipped).  Ranks own contiguous nnz-balanced ranges in ascending row order (the
 * reference's bucket split, distributed/scheduler/RunOneTask.cpp:160-243). */
int qmfx_dist_plan(const int64_t* rowptr, int64_t nrows, int world, int npieces,
                   int64_t* pbounds);

/* ---- measurement -------------------------------------------------------------------------- */
/* HIP-event time of the row-solve kernel launches (on the context stream) since reset; the
 * kernels of qmfx_bpr_epoch, qmfx_recommend and qmfx_similar calls are counted here too (one
 * unit of a similar call is 2k flop per (query, row) pair), and those of the fold-in calls
 * (planning and gather included; the work counted is the k×k form of every row), and those of
 * the explanation calls (the work formula stands with qmfx_wals_explain), and those of the BPR
 * fold-in calls (the work formula stands with qmfx_bpr_fold_in). */
int qmfx_solve_kernel_stats(qmfx_ctx* ctx, double* total_ms, int64_t* launches,
                            double* flops, double* bytes);
/* Per kernel class since reset: 0 = direct row kernel, 1 = whitened row kernels (row solve
 * + unwhitening GEMM), 2 = whole half-epoch (all kernels, collectives included).  flops /
 * bytes are the algorithmic work of that class (SURVEY.md §8(d) accounting). */
int qmfx_kernel_stats(qmfx_ctx* ctx, int cls, double* total_ms, int64_t* launches,
                      double* flops, double* bytes);
/* qmfx_kernel_stats restricted to the halves that solved `side` (0 users, 1 items): a class's
 * launches differ by side, so the per-launch time of the class's large launch is read here. */
int qmfx_kernel_stats_side(qmfx_ctx* ctx, int cls, int side, double* total_ms, int64_t* launches,
                           double* flops, double* bytes);
int qmfx_reset_stats(qmfx_ctx* ctx);
/* Multi-rank halves (qmfx_dist_init with a communicator) that solved `side`, since reset:
 * exchange_ms = Σ time of the per-piece broadcast groups on the collective stream (HIP events
 * there; a piece's group starts when its solves are done and the previous group finished);
 * exposed_ms = Σ from the last piece's solves done to its broadcasts done (the exchange not
 * hidden behind solves); solve_ms = Σ row-solve time of the pieces.  Zero on one rank. */
int qmfx_exchange_stats(qmfx_ctx* ctx, int side, double* exchange_ms, double* exposed_ms,
                        double* solve_ms, int64_t* halves);
/* The last qmfx_bpr_epoch's launch plan: concurrent waves (Hogwild width) and whether the user
 * row's change was added atomically (1: a heavy user makes concurrent holders likely) or
 * stored (0). */
int qmfx_bpr_plan(qmfx_ctx* ctx, int* waves, int* atomic_user);
/* "" for the product library; a timing-variant build (tools/build_variant.sh) returns its
 * compile flags, so a variant loaded through QMFX_LIB is never taken for the product. */
const char* qmfx_build_variant(void);

/* ---- self tests ------------------------------------------------------------------------------ */
/* C(16×16) = A(16×4)·B(4×16) through the kernels' MFMA operand/accumulator maps. */
int qmfx_selftest_mfma(int device, int precision, const double* A, const double* B, double* C);

#ifdef __cplusplus
}
#endif
#endif /* QMFX_H_ */
