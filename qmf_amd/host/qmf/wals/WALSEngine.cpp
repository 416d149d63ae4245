#include <qmf/wals/WALSEngine.h>

#include <algorithm>
#include <fstream>
#include <limits>
#include <random>

#include <qmf/Matrix.h>
#include <qmf/utils/Log.h>

namespace qmf {

WALSEngine::WALSEngine(const WALSConfig& config,
                       const std::unique_ptr<MetricsEngine>& metricsEngine,
                       const size_t nthreads,
                       const DeviceOptions& device)
    : config_(config), metricsEngine_(metricsEngine), deviceOptions_(device),
      parallel_(nthreads) {
  if (metricsEngine_ && !metricsEngine_->testAvgMetrics().empty() &&
      metricsEngine_->config().numTestUsers == 0) {
    LOG(WARNING) << "computing average test metrics on all users can be slow! "
                    "Set numTestUsers > 0 to sample some of them";
  }
}

WALSEngine::~WALSEngine() = default;

void WALSEngine::init(const std::vector<DatasetElem>& dataset) {
  CHECK(!userFactors_ && !itemFactors_) << "engine was already initialized with train data";
  CHECK_GT(config_.nfactors, 0);
  CHECK(!dataset.empty()) << "empty train dataset";
  CHECK_GE(deviceOptions_.ngpus, 1) << "--ngpus must be at least 1";
  if (deviceOptions_.ngpus > 1) {
    int visible = 0;
    QMFX_CHECK(qmfx_device_count(&visible));
    CHECK_LE(deviceOptions_.device + deviceOptions_.ngpus, visible)
        << "--ngpus " << deviceOptions_.ngpus << " from --device " << deviceOptions_.device
        << " needs " << deviceOptions_.device + deviceOptions_.ngpus << " GPUs; " << visible
        << " visible";
  }
  dev_ = std::make_unique<DeviceContext>(deviceOptions_, config_.nfactors);
  ranks_.assign(1, dev_->get());
  for (int r = 1; r < deviceOptions_.ngpus; ++r) {
    peers_.push_back(std::make_unique<DeviceContext>(deviceOptions_, config_.nfactors, r));
    ranks_.push_back(peers_.back()->get());
  }
  qmfx_ctx* c = dev_->get();
  if (dataset.size() < static_cast<size_t>(std::numeric_limits<int32_t>::max())) {
    // ids, idx and both CSR orientations built on the device (qmfx_group_signals)
    int64_t nu = 0, ni = 0;
    QMFX_CHECK(qmfx_group_signals(c, dataset.data(), static_cast<int64_t>(dataset.size()), &nu,
                                  &ni));
    std::vector<int64_t> uids(static_cast<size_t>(nu)), iids(static_cast<size_t>(ni));
    QMFX_CHECK(qmfx_get_ids(c, QMFX_USERS, uids.data()));
    QMFX_CHECK(qmfx_get_ids(c, QMFX_ITEMS, iids.data()));
    userIndex_.assignSorted(std::move(uids));
    itemIndex_.assignSorted(std::move(iids));
    // the other ranks copy rank 0's CSR device to device over xGMI (one sort, no further
    // host→device uploads); qmfx_dist_init_all then keeps each rank's shard
    for (size_t r = 1; r < ranks_.size(); ++r) QMFX_CHECK(qmfx_import_signals(ranks_[r], c));
  } else {
    // beyond the device sort's 32-bit item count: the same grouping on the host
    SignalCsr byUser, byItem;
    groupSignals(dataset, userIndex_, itemIndex_, byUser, byItem, parallel_.nthreads());
    for (qmfx_ctx* rc : ranks_) {
      QMFX_CHECK(qmfx_set_shape(rc, static_cast<int64_t>(nusers()),
                                static_cast<int64_t>(nitems())));
      QMFX_CHECK(qmfx_upload_csr(rc, QMFX_USERS, byUser.rowptr.data(), byUser.col.data(),
                                 byUser.val.data(), static_cast<int64_t>(byUser.nnz())));
      QMFX_CHECK(qmfx_upload_csr(rc, QMFX_ITEMS, byItem.rowptr.data(), byItem.col.data(),
                                 byItem.val.data(), static_cast<int64_t>(byItem.nnz())));
    }
  }

  userFactors_ = std::make_unique<FactorData>(nusers(), config_.nfactors);
  itemFactors_ = std::make_unique<FactorData>(nitems(), config_.nfactors);
  if (config_.DistributionFile.empty()) {
    // not reproducible by design (random_device), as in the reference (WALSEngine.cpp:56-63)
    std::random_device rd;
    std::mt19937 gen(rd());
    std::uniform_real_distribution<Double> distr(-config_.initDistributionBound,
                                                 config_.initDistributionBound);
    itemFactors_->setFactors([&](auto...) { return distr(gen); });
  } else {
    itemFactors_->setFactors(config_.DistributionFile);
  }

  for (qmfx_ctx* rc : ranks_) {
    QMFX_CHECK(qmfx_set_factors(rc, QMFX_USERS, userFactors_->getFactors().data()));
    QMFX_CHECK(qmfx_set_factors(rc, QMFX_ITEMS, itemFactors_->getFactors().data()));
  }
  if (ranks_.size() > 1) {
    QMFX_CHECK(qmfx_dist_init_all(ranks_.data(), static_cast<int>(ranks_.size())));
    LOG(INFO) << "rows partitioned over " << ranks_.size() << " GPUs (devices "
              << deviceOptions_.device << ".." << deviceOptions_.device + ranks_.size() - 1
              << "), RCCL all-gather per half-epoch";
  }
  hostStale_ = false;
}

void WALSEngine::initTest(const std::vector<DatasetElem>& testDataset) {
  CHECK(testUsers_.empty()) << "engine was already initialized with test data";
  if (metricsEngine_ && !metricsEngine_->testAvgMetrics().empty()) {
    initAvgTestData(testUsers_, testLabels_, testScores_, testDataset, userIndex_, itemIndex_,
                    metricsEngine_->config().numTestUsers, metricsEngine_->config().seed);
  }
}

void WALSEngine::reportFailedRows(const int side) {
  int64_t count = 0;
  for (qmfx_ctx* rc : ranks_) {  // each rank flags the rows it solved
    int64_t n = 0;
    QMFX_CHECK(qmfx_wals_failed_rows(rc, nullptr, 0, &n));
    count += n;
  }
  if (count == 0) return;
  if (config_.cgSteps > 0) {
    // conjugate gradients are defined for positive definite systems only: no re-solve
    LOG(WARNING) << count << (side == QMFX_USERS ? " user" : " item")
                 << " systems are not positive definite; stopped at their last iterate";
    return;
  }
  // the device re-solved them in fp64 with a pivoted factorization (dsysv_'s role,
  // Matrix.cpp:81-96) inside the half; a singular one fails qmfx_wals_half itself
  LOG(WARNING) << count << (side == QMFX_USERS ? " user" : " item")
               << " systems are not positive definite; re-solved with pivoting on the device";
  pivotedRows_ += static_cast<size_t>(count);
}

Double WALSEngine::iterate(const int side) {
  Double sum = 0.0;
  if (ranks_.size() > 1)
    QMFX_CHECK(qmfx_wals_half_multi(ranks_.data(), static_cast<int>(ranks_.size()), side,
                                    config_.confidenceWeight, config_.regularizationLambda, &sum));
  else if (config_.cgSteps > 0)
    QMFX_CHECK(qmfx_wals_half_cg(dev_->get(), side, config_.confidenceWeight,
                                 config_.regularizationLambda, static_cast<int>(config_.cgSteps),
                                 &sum));
  else
    QMFX_CHECK(qmfx_wals_half(dev_->get(), side, config_.confidenceWeight,
                              config_.regularizationLambda, &sum));
  reportFailedRows(side);
  hostStale_ = true;
  lastLoss_ = sum / (static_cast<Double>(nusers()) * static_cast<Double>(nitems()));
  return lastLoss_;
}

void WALSEngine::optimize() {
  CHECK(userFactors_ && itemFactors_) << "no factor data, have you initialized the engine?";
  for (size_t epoch = 1; epoch <= config_.nepochs; ++epoch) {
    iterate(QMFX_USERS);                    // item factors fixed
    const Double loss = iterate(QMFX_ITEMS);  // user factors fixed
    LOG(INFO) << "epoch " << epoch << ": train loss = " << loss;
    evaluate(epoch);
  }
  for (qmfx_ctx* rc : ranks_) QMFX_CHECK(qmfx_sync(rc));
}

void WALSEngine::syncHost() const {
  if (!hostStale_ || !dev_) return;
  QMFX_CHECK(qmfx_get_factors(dev_->get(), QMFX_USERS, userFactors_->getFactors().data()));
  QMFX_CHECK(qmfx_get_factors(dev_->get(), QMFX_ITEMS, itemFactors_->getFactors().data()));
  hostStale_ = false;
}

void WALSEngine::evaluate(const size_t epoch) {
  if (metricsEngine_ && !metricsEngine_->testAvgMetrics().empty() && !testUsers_.empty() &&
      (metricsEngine_->config().alwaysCompute || epoch == config_.nepochs)) {
    LOG(INFO) << "do compute evaluate ...";
    computeTestRanks(dev_->get(), false, testUsers_, testLabels_, testRanks_);
    metricsEngine_->computeAndRecordTestAvgMetrics(epoch, testRanks_, parallel_);
  }
}

const FactorData& WALSEngine::userFactors() const {
  CHECK(userFactors_) << "user factors wasn't initialized";
  syncHost();
  return *userFactors_;
}

const FactorData& WALSEngine::itemFactors() const {
  CHECK(itemFactors_) << "item factors wasn't initialized";
  syncHost();
  return *itemFactors_;
}

void WALSEngine::saveUserFactors(const std::string& fileName) const {
  saveFactors(userFactors(), userIndex_, fileName);
}

void WALSEngine::saveItemFactors(const std::string& fileName) const {
  saveFactors(itemFactors(), itemIndex_, fileName);
}

void WALSEngine::saveUserRecommendations(const std::string& fileName, const size_t topN,
                                         const bool includeSeen,
                                         const std::vector<int64_t>* userIds,
                                         const RecommendScope& scope) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  // a rank holds only its own users' signals; routing users to their rank is not built
  CHECK_EQ(ranks_.size(), 1u) << "recommendations need --ngpus=1";
  saveRecommendations(dev_->get(), includeSeen ? QMFX_REC_ALL : QMFX_REC_UNSEEN_SIGNALS, false,
                      userIndex_, itemIndex_, fileName, topN, userIds, nullptr, scope);
}

namespace {

// the (user, item) pairs of a batch's recommendation lists as explain queries: query t
// explains targets[qptr[t] .. qptr[t + 1]); pairRows[p] = rows[t] of pair p's query
void listsToQueries(const int64_t* rows, const size_t n, const size_t topN, const int64_t* items,
                    const int32_t* counts, std::vector<int64_t>& qptr,
                    std::vector<int64_t>& targets, std::vector<int64_t>& pairRows) {
  qptr.assign(n + 1, 0);
  targets.clear();
  pairRows.clear();
  for (size_t t = 0; t < n; ++t) {
    for (int32_t r = 0; r < counts[t]; ++r) {
      targets.push_back(items[t * topN + static_cast<size_t>(r)]);
      pairRows.push_back(rows[t]);
    }
    qptr[t + 1] = static_cast<int64_t>(targets.size());
  }
}

struct ExplainLists {
  std::vector<int64_t> sources, positions;
  std::vector<double> contribs, totals;
  std::vector<int32_t> counts;
  ExplainLists(const size_t npairs, const size_t topM)
      : sources(npairs * topM), positions(npairs * topM), contribs(npairs * topM),
        totals(npairs), counts(npairs) {}
};

}  // namespace

void WALSEngine::saveRecommendationExplanations(const std::string& recommendationsFile,
                                                const std::string& explanationsFile,
                                                const size_t topN, const size_t topM,
                                                const bool includeSeen,
                                                const std::vector<int64_t>* userIds,
                                                const RecommendScope& scope) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  CHECK_EQ(ranks_.size(), 1u) << "recommendations need --ngpus=1";
  CHECK(topM >= 1 && topM <= QMFX_REC_MAX_N)
      << "the number of explanations must be in 1.." << QMFX_REC_MAX_N << ", got " << topM;
  qmfx_ctx* c = dev_->get();
  const Double alpha = config_.confidenceWeight, lambda = config_.regularizationLambda;
  std::ofstream eout(explanationsFile);
  std::vector<int64_t> qptr, targets, pairRows;
  const AfterBatch after = [&](const int64_t* rows, const size_t n, const int64_t* items,
                               const int32_t* counts) {
    listsToQueries(rows, n, topN, items, counts, qptr, targets, pairRows);
    if (targets.empty()) return;
    ExplainLists x(targets.size(), topM);
    QMFX_CHECK(qmfx_wals_explain(c, QMFX_USERS, static_cast<int64_t>(n), rows, qptr.data(),
                                 targets.data(), alpha, lambda, static_cast<int>(topM),
                                 x.sources.data(), x.positions.data(), x.contribs.data(),
                                 x.counts.data(), x.totals.data(), nullptr));
    writeExplanations(userIndex_, itemIndex_, pairRows, targets, topM, x.sources.data(),
                      x.contribs.data(), x.counts.data(), eout);
  };
  saveRecommendations(c, includeSeen ? QMFX_REC_ALL : QMFX_REC_UNSEEN_SIGNALS, false, userIndex_,
                      itemIndex_, recommendationsFile, topN, userIds, &after, scope);
}

void WALSEngine::saveItemSimilarities(const std::string& fileName, const size_t topN,
                                  const bool cosine, const std::vector<int64_t>* itemIds) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  saveSimilarities(dev_->get(), QMFX_ITEMS, itemIndex_, fileName, topN, cosine, itemIds);
}

void WALSEngine::saveUserSimilarities(const std::string& fileName, const size_t topN,
                                  const bool cosine, const std::vector<int64_t>* userIds) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  saveSimilarities(dev_->get(), QMFX_USERS, userIndex_, fileName, topN, cosine, userIds);
}

size_t WALSEngine::foldInUsers(const std::vector<DatasetElem>& lines,
                               const std::string& userFactorsFile,
                               const std::string& recommendationsFile, const size_t topN,
                               const bool includeSeen, const std::string& explanationsFile,
                               const size_t topM) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  if (!explanationsFile.empty()) {
    CHECK(!recommendationsFile.empty()) << "fold-in explanations need the recommendations file";
    CHECK(topM >= 1 && topM <= QMFX_REC_MAX_N)
        << "the number of explanations must be in 1.." << QMFX_REC_MAX_N << ", got " << topM;
  }
  if (!recommendationsFile.empty())
    CHECK(topN >= 1 && topN <= QMFX_REC_MAX_N)
        << "the number of recommendations must be in 1.." << QMFX_REC_MAX_N << ", got " << topN;
  // (user id, item idx, value) of the lines whose item the model knows
  struct Signal {
    int64_t user;
    int32_t item;
    Double value;
  };
  std::vector<Signal> signals;
  signals.reserve(lines.size());
  size_t unknown = 0;
  for (const auto& e : lines) {
    const size_t i = itemIndex_.idx(e.itemId);
    if (i == IdIndex::missingIdx)
      ++unknown;
    else
      signals.push_back(Signal{e.userId, static_cast<int32_t>(i), e.value});
  }
  if (unknown > 0)
    LOG(WARNING) << unknown << " fold-in lines name items that are not in the training data; dropped";
  std::stable_sort(signals.begin(), signals.end(), [](const Signal& a, const Signal& b) {
    return a.user != b.user ? a.user < b.user : a.item < b.item;
  });
  std::vector<int64_t> ids, rowptr(1, 0);
  std::vector<int32_t> col(signals.size());
  std::vector<Double> val(signals.size());
  for (size_t e = 0; e < signals.size(); ++e) {
    if (e == 0 || signals[e].user != signals[e - 1].user) {
      if (e > 0) rowptr.push_back(static_cast<int64_t>(e));
      ids.push_back(signals[e].user);
    }
    col[e] = signals[e].item;
    val[e] = signals[e].value;
  }
  if (!signals.empty()) rowptr.push_back(static_cast<int64_t>(signals.size()));
  const size_t n = ids.size(), k = config_.nfactors;
  if (n == 0) {
    LOG(WARNING) << "no fold-in user has a signal on a known item; nothing folded in";
    if (!userFactorsFile.empty()) std::ofstream(userFactorsFile).flush();
    if (!recommendationsFile.empty()) std::ofstream(recommendationsFile).flush();
    if (!explanationsFile.empty()) std::ofstream(explanationsFile).flush();
    return 0;
  }
  IdIndex index;
  index.assignSorted(std::move(ids));
  FactorData folded(n, k);
  qmfx_ctx* c = dev_->get();
  const Double alpha = config_.confidenceWeight, lambda = config_.regularizationLambda;
  if (recommendationsFile.empty()) {
    int64_t pivoted = 0;
    QMFX_CHECK(qmfx_wals_fold_in(c, QMFX_USERS, static_cast<int64_t>(n), rowptr.data(), col.data(),
                                 val.data(), alpha, lambda, folded.getFactors().data(), nullptr,
                                 &pivoted));
    if (pivoted > 0)
      LOG(WARNING) << pivoted
                   << " fold-in systems are not positive definite; re-solved with pivoting on the device";
  } else {
    std::vector<int64_t> items(n * topN), rows(n);
    std::vector<double> scores(n * topN);
    std::vector<int32_t> counts(n);
    for (size_t r = 0; r < n; ++r) rows[r] = static_cast<int64_t>(r);
    QMFX_CHECK(qmfx_recommend_fold_in(c, static_cast<int64_t>(n), rowptr.data(), col.data(),
                                      val.data(), alpha, lambda, static_cast<int>(topN),
                                      includeSeen ? 0 : 1, items.data(), scores.data(),
                                      counts.data(), folded.getFactors().data()));
    std::string text;
    formatPairs(index, itemIndex_, rows.data(), 0, n, topN, items.data(), scores.data(),
                counts.data(), text);
    std::ofstream fout(recommendationsFile);
    fout.write(text.data(), static_cast<std::streamsize>(text.size()));
    if (!explanationsFile.empty()) {
      std::ofstream eout(explanationsFile);
      std::vector<int64_t> qptr, targets, pairRows;
      listsToQueries(rows.data(), n, topN, items.data(), counts.data(), qptr, targets, pairRows);
      if (!targets.empty()) {
        ExplainLists x(targets.size(), topM);
        QMFX_CHECK(qmfx_wals_explain_rows(c, QMFX_USERS, static_cast<int64_t>(n), rowptr.data(),
                                          col.data(), val.data(), qptr.data(), targets.data(),
                                          alpha, lambda, static_cast<int>(topM), x.sources.data(),
                                          x.positions.data(), x.contribs.data(), x.counts.data(),
                                          x.totals.data(), nullptr));
        writeExplanations(index, itemIndex_, pairRows, targets, topM, x.sources.data(),
                          x.contribs.data(), x.counts.data(), eout);
      }
    }
  }
  if (!userFactorsFile.empty()) saveFactors(folded, index, userFactorsFile);
  return n;
}

size_t WALSEngine::nusers() const { return userIndex_.size(); }
size_t WALSEngine::nitems() const { return itemIndex_.size(); }

}  // namespace qmf
