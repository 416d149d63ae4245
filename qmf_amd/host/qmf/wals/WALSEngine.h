// Implicit-feedback ALS engine, drop-in for the reference's qmf::WALSEngine
// (qmf/wals/WALSEngine.h:35-143, WALSEngine.cpp:24-355).  Same constructor, methods,
// logging and output files; the epoch loop runs on an MI355X through the qmfx C ABI
// (include/qmfx.h): both CSR orientations and both factor matrices stay resident in HBM,
// one qmfx_wals_half call per half-epoch.  The host keeps the id indexes and a mirror of
// the factors that is refreshed when something reads it (evaluation, saving).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include <qmf/Device.h>
#include <qmf/Engine.h>
#include <qmf/FactorData.h>
#include <qmf/Types.h>
#include <qmf/metrics/MetricsEngine.h>
#include <qmf/utils/IdIndex.h>
#include <qmf/utils/ParallelExecutor.h>
#include <qmf/wals/Signals.h>

namespace qmf {

struct WALSConfig {
  size_t nepochs;
  size_t nfactors;
  Double regularizationLambda;
  Double confidenceWeight;
  Double initDistributionBound;
  std::string DistributionFile;
  // 0: every row is solved exactly; N > 0: N warm-started conjugate-gradient steps per row
  // and half (qmfx_wals_half_cg; one device)
  size_t cgSteps = 0;
};

class WALSEngine : public Engine {
 public:
  // `config` and `metricsEngine` are kept by reference (caller-owned), as in the reference.
  // `nthreads` sizes the host-side work (ingest, evaluation, output formatting).
  explicit WALSEngine(const WALSConfig& config,
                      const std::unique_ptr<MetricsEngine>& metricsEngine,
                      const size_t nthreads = 16,
                      const DeviceOptions& device = DeviceOptions());
  ~WALSEngine() override;

  void init(const std::vector<DatasetElem>& dataset) override;
  void initTest(const std::vector<DatasetElem>& testDataset) override;
  void optimize() override;
  void evaluate(const size_t epoch) override;

  size_t nusers() const;
  size_t nitems() const;

  void saveUserFactors(const std::string& fileName) const override;
  void saveItemFactors(const std::string& fileName) const override;
  // includeSeen = false leaves out the items of the user's training signals (one GPU only)
  void saveUserRecommendations(const std::string& fileName, size_t topN, bool includeSeen,
                               const std::vector<int64_t>* userIds = nullptr,
                               const RecommendScope& scope = RecommendScope()) const override;
  // saveUserRecommendations to recommendationsFile, and to explanationsFile why: for every
  // (user, item) pair of that file, in its order, the topM (1..QMFX_REC_MAX_N) training signals
  // of the user that contribute most to y_itemᵀA_u⁻¹b_u (include/qmfx.h qmfx_wals_explain, the
  // config's α and λ), one line "<userId> <itemId> <sourceItemId> <contribution>\n" (%.9f) per
  // source, in rank order.  The contributions of a pair add up to the score of the user solved
  // from the current item factors, which is not the recommendation's score (the stored user
  // row was solved before the last item half).  Needs positive definite systems: the device
  // refuses (and this aborts) when a user has a signal with 1 + αv < 0.  One GPU only.
  void saveRecommendationExplanations(const std::string& recommendationsFile,
                                      const std::string& explanationsFile, size_t topN,
                                      size_t topM, bool includeSeen,
                                      const std::vector<int64_t>* userIds = nullptr,
                                      const RecommendScope& scope = RecommendScope()) const;
  // the query itself is always left out; with several GPUs rank 0 answers (full replicas)
  void saveItemSimilarities(const std::string& fileName, size_t topN, bool cosine,
                            const std::vector<int64_t>* itemIds = nullptr) const override;
  void saveUserSimilarities(const std::string& fileName, size_t topN, bool cosine,
                            const std::vector<int64_t>* userIds = nullptr) const override;

  // Fold-in (addition to the reference API): the users of `lines` are solved as new rows from
  // these signals against the trained item factors (qmfx_wals_fold_in, rank 0, config's α and
  // λ), whether or not their id was trained; the model is left as it is.  Lines are grouped by
  // user id, ascending, with each user's items ascending; a line naming an item that is not in
  // the training data is dropped, and their number is logged once as a warning.
  // userFactorsFile (unless empty): "<id> <f0> … <fk-1>" per new user, saveUserFactors' format.
  // recommendationsFile (unless empty): saveUserRecommendations' format for the new users,
  // topN per user; includeSeen = false leaves out the items of the user's own lines.
  // explanationsFile (unless empty; needs recommendationsFile): saveRecommendationExplanations'
  // format for the pairs of recommendationsFile, topM sources per pair, from the new users' own
  // lines (qmfx_wals_explain_rows); here a pair's contributions add up to its score.
  // Returns the number of users folded in.
  size_t foldInUsers(const std::vector<DatasetElem>& lines, const std::string& userFactorsFile,
                     const std::string& recommendationsFile, size_t topN, bool includeSeen,
                     const std::string& explanationsFile = "", size_t topM = 5) const;

  // --- additions (not in the reference API) ---
  // host copies of the current factors (synchronised from the device on access)
  const FactorData& userFactors() const;
  const FactorData& itemFactors() const;
  const IdIndex& userIndex() const { return userIndex_; }
  const IdIndex& itemIndex() const { return itemIndex_; }
  // the loss the last half-epoch returned (Σ row losses / (nusers · nitems))
  Double lastLoss() const { return lastLoss_; }
  // rows re-solved with pivoting (on the device) because their system was not positive
  // definite
  size_t pivotedRows() const { return pivotedRows_; }
  qmfx_ctx* deviceContext() const { return dev_ ? dev_->get() : nullptr; }

 private:
  // one half-epoch: solve every row of `side` with the other side fixed; returns the
  // loss normalised as WALSEngine::iterate does (WALSEngine.cpp:215)
  Double iterate(int side);
  // logs the rows of the last half whose system was not positive definite (the device
  // re-solved them with pivoting inside the half)
  void reportFailedRows(int side);
  void syncHost() const;

  const WALSConfig& config_;
  const std::unique_ptr<MetricsEngine>& metricsEngine_;
  DeviceOptions deviceOptions_;
  mutable ParallelExecutor parallel_;
  std::unique_ptr<DeviceContext> dev_;
  // --ngpus > 1: the other ranks' contexts (dev_ is rank 0); all are passed to
  // qmfx_wals_half_multi in rank order
  std::vector<std::unique_ptr<DeviceContext>> peers_;
  std::vector<qmfx_ctx*> ranks_;

  IdIndex userIndex_;
  IdIndex itemIndex_;
  mutable std::unique_ptr<FactorData> userFactors_;
  mutable std::unique_ptr<FactorData> itemFactors_;
  mutable bool hostStale_ = false;

  std::vector<size_t> testUsers_;
  std::vector<std::vector<Double>> testLabels_;
  std::vector<std::vector<Double>> testScores_;
  std::vector<RankedUser> testRanks_;

  Double lastLoss_ = 0.0;
  size_t pivotedRows_ = 0;
};

}  // namespace qmf
