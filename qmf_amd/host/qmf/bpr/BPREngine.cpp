#include <qmf/bpr/BPREngine.h>

#include <algorithm>
#include <fstream>

#include <qmf/utils/Log.h>

namespace qmf {

BPREngine::BPREngine(const BPRConfig& config,
                     const std::unique_ptr<MetricsEngine>& metricsEngine,
                     const size_t evalNumNeg,
                     const int32_t evalSeed,
                     const size_t nthreads,
                     const DeviceOptions& device)
    : config_(config), metricsEngine_(metricsEngine), evalNumNeg_(evalNumNeg),
      evalSeed_(evalSeed), deviceOptions_(device), parallel_(nthreads),
      gen_(std::random_device()()) {
  if (config_.numHogwildThreads > nthreads) {
    LOG(WARNING) << "number of hogwild threads should be smaller than number of "
                    "threads in the threadpool";
  }
  if (metricsEngine_ && !metricsEngine_->testAvgMetrics().empty() &&
      metricsEngine_->config().numTestUsers == 0) {
    LOG(WARNING) << "computing average test metrics on all users can be slow! "
                    "Set numTestUsers > 0 to sample some of them";
  }
}

BPREngine::~BPREngine() = default;

size_t BPREngine::nusers() const { return userIndex_.size(); }
size_t BPREngine::nitems() const { return itemIndex_.size(); }

BPREngine::PositiveSets BPREngine::buildSets(const std::vector<std::pair<size_t, size_t>>& pairs,
                                             const size_t nusers) {
  PositiveSets s;
  s.rowptr.assign(nusers + 1, 0);
  for (const auto& p : pairs) ++s.rowptr[p.first + 1];
  for (size_t u = 0; u < nusers; ++u) s.rowptr[u + 1] += s.rowptr[u];
  std::vector<int64_t> fill(s.rowptr.begin(), s.rowptr.end() - 1);
  s.items.resize(pairs.size());
  for (const auto& p : pairs) s.items[fill[p.first]++] = p.second;
  // sort + dedupe each row, then compact
  int64_t w = 0;
  for (size_t u = 0; u < nusers; ++u) {
    const int64_t b = s.rowptr[u], e = s.rowptr[u + 1];
    std::sort(s.items.begin() + b, s.items.begin() + e);
    const int64_t n = std::unique(s.items.begin() + b, s.items.begin() + e) - (s.items.begin() + b);
    std::move(s.items.begin() + b, s.items.begin() + b + n, s.items.begin() + w);
    s.rowptr[u] = w;
    w += n;
  }
  s.rowptr[nusers] = w;
  s.items.resize(static_cast<size_t>(w));
  return s;
}

bool BPREngine::PositiveSets::contains(const size_t u, const size_t i) const {
  return std::binary_search(items.begin() + rowptr[u], items.begin() + rowptr[u + 1], i);
}

size_t BPREngine::sampleRandomNegative(const size_t userIdx, std::mt19937& gen,
                                       const PositiveSets& sets) const {
  // the reference would spin forever here; abort instead
  CHECK_LT(sets.count(userIdx), nitems()) << "user idx " << userIdx
                                          << " has every item as a positive";
  std::uniform_int_distribution<> dis(0, static_cast<int>(nitems()) - 1);
  size_t neg;
  do {
    neg = dis(gen);
  } while (sets.contains(userIdx, neg));
  return neg;
}

void BPREngine::init(const std::vector<DatasetElem>& dataset) {
  initHost(dataset);
  initDevice();
}

void BPREngine::initHost(const std::vector<DatasetElem>& dataset) {
  CHECK(!userFactors_ && !itemFactors_) << "engine was already initialized with train data";
  for (const auto& e : dataset) {
    if (e.value < 1.0) continue;
    const size_t u = userIndex_.getOrSetIdx(e.userId);
    const size_t i = itemIndex_.getOrSetIdx(e.itemId);
    data_.emplace_back(u, i);
  }
  itemMap_ = buildSets(data_, nusers());

  // evaluation set: every positive × evalNumNeg negatives, mt19937(evalSeed)
  {
    std::mt19937 gen(evalSeed_);
    evalSet_.reserve(data_.size() * evalNumNeg_);
    for (const auto& p : data_)
      for (size_t j = 0; j < evalNumNeg_; ++j)
        evalSet_.push_back(PosNegTriplet{p.first, p.second,
                                         sampleRandomNegative(p.first, gen, itemMap_)});
  }

  learningRate_ = config_.initLearningRate;
  userFactors_ = std::make_unique<FactorData>(nusers(), config_.nfactors);
  itemFactors_ = std::make_unique<FactorData>(nitems(), config_.nfactors, config_.useBiases);
  std::uniform_real_distribution<Double> distr(-config_.initDistributionBound,
                                               config_.initDistributionBound);
  auto unif = [&](auto...) { return distr(gen_); };
  userFactors_->setFactors(unif);
  itemFactors_->setFactors(unif);
  if (config_.useBiases) itemFactors_->setBiases(unif);
}

void BPREngine::initDevice() {
  // Hogwild across GPUs would need cross-device atomics: BPR runs on one GPU (replicas only)
  CHECK_EQ(deviceOptions_.ngpus, 1) << "BPR runs on one GPU (QMF_NGPUS / --ngpus is WALS only)";
  dev_ = std::make_unique<DeviceContext>(deviceOptions_, config_.nfactors);
  qmfx_ctx* c = dev_->get();
  QMFX_CHECK(qmfx_set_shape(c, static_cast<int64_t>(nusers()), static_cast<int64_t>(nitems())));
  std::vector<int64_t> pu(data_.size()), pi(data_.size());
  for (size_t e = 0; e < data_.size(); ++e) {
    pu[e] = static_cast<int64_t>(data_[e].first);
    pi[e] = static_cast<int64_t>(data_[e].second);
  }
  QMFX_CHECK(qmfx_bpr_set_positives(c, pu.data(), pi.data(), static_cast<int64_t>(pu.size())));
  QMFX_CHECK(qmfx_set_factors(c, QMFX_USERS, userFactors_->getFactors().data()));
  QMFX_CHECK(qmfx_set_factors(c, QMFX_ITEMS, itemFactors_->getFactors().data()));
  std::vector<Double> zeros;
  const Double* bias = itemFactors_->getBiases().data();
  if (!config_.useBiases) {
    zeros.assign(nitems(), 0.0);
    bias = zeros.data();
  }
  QMFX_CHECK(qmfx_bpr_set_biases(c, bias));
  hostStale_ = false;
}

void BPREngine::initTest(const std::vector<DatasetElem>& testDataset) {
  CHECK(testEvalSet_.empty()) << "engine was already initialzied with test data";
  std::vector<std::pair<size_t, size_t>> valid;
  valid.reserve(testDataset.size());
  for (const auto& e : testDataset) {
    if (e.value < 1.0) continue;
    const size_t u = userIndex_.idx(e.userId);
    const size_t i = itemIndex_.idx(e.itemId);
    if (u == IdIndex::missingIdx || i == IdIndex::missingIdx) continue;
    valid.emplace_back(u, i);
  }
  testItemMap_ = buildSets(valid, nusers());
  std::mt19937 gen(evalSeed_);
  testEvalSet_.reserve(evalNumNeg_ * valid.size());
  for (const auto& p : valid)
    for (size_t j = 0; j < evalNumNeg_; ++j)
      testEvalSet_.push_back(PosNegTriplet{p.first, p.second,
                                           sampleRandomNegative(p.first, gen, testItemMap_)});
  if (metricsEngine_ && !metricsEngine_->testAvgMetrics().empty()) {
    initAvgTestData(testUsers_, testLabels_, testScores_, testDataset, userIndex_, itemIndex_,
                    metricsEngine_->config().numTestUsers, metricsEngine_->config().seed);
  }
}

void BPREngine::optimize() {
  CHECK(userFactors_ && itemFactors_) << "no factor data, have you initialized the engine?";
  for (size_t epoch = 1; epoch <= config_.nepochs; ++epoch) {
    // the reference visits positives in file order in epoch 1 and shuffles after each
    // epoch; the device kernel visits them in a seeded permutation from epoch 2 on
    const uint64_t seed = (static_cast<uint64_t>(gen_()) << 32) | gen_();
    const int shuffle = config_.shuffleTrainingSet && epoch > 1 ? 1 : 0;
    QMFX_CHECK(qmfx_bpr_epoch(dev_->get(), seed, static_cast<int>(config_.numNegativeSamples),
                              learningRate_, config_.biasLambda, config_.userLambda,
                              config_.itemLambda, config_.useBiases ? 1 : 0, shuffle));
    hostStale_ = true;
    evaluate(epoch);
    if (config_.decayRate < 1.0) learningRate_ *= config_.decayRate;
  }
  QMFX_CHECK(qmfx_sync(dev_->get()));
}

Double BPREngine::evalLoss(const int slot, const std::vector<PosNegTriplet>& set) const {
  if (set.empty()) return -1.0;
  Double sum = 0.0;
  QMFX_CHECK(qmfx_bpr_eval(dev_->get(), slot, reinterpret_cast<const int64_t*>(set.data()),
                           static_cast<int64_t>(set.size()), config_.useBiases ? 1 : 0, &sum));
  return sum / set.size();
}

void BPREngine::evaluate(const size_t epoch) {
  // mean log(1 + exp(−x̂)) over the fixed evaluation triplets (BPREngine.cpp:246-264)
  lastTrainLoss_ = evalLoss(0, evalSet_);
  lastTestLoss_ = evalLoss(1, testEvalSet_);
  LOG(INFO) << "epoch " << epoch << ": train loss = " << lastTrainLoss_
            << ", test loss = " << lastTestLoss_;
  if (metricsEngine_ && !metricsEngine_->testAvgMetrics().empty() && !testUsers_.empty() &&
      (metricsEngine_->config().alwaysCompute || epoch == config_.nepochs)) {
    computeTestRanks(dev_->get(), itemFactors_->withBiases(), testUsers_, testLabels_, testRanks_);
    metricsEngine_->computeAndRecordTestAvgMetrics(epoch, testRanks_, parallel_);
  }
}

void BPREngine::syncHost() const {
  if (!hostStale_ || !dev_) return;
  QMFX_CHECK(qmfx_get_factors(dev_->get(), QMFX_USERS, userFactors_->getFactors().data()));
  QMFX_CHECK(qmfx_get_factors(dev_->get(), QMFX_ITEMS, itemFactors_->getFactors().data()));
  if (config_.useBiases)
    QMFX_CHECK(qmfx_bpr_get_biases(dev_->get(), itemFactors_->getBiases().data()));
  hostStale_ = false;
}

const FactorData& BPREngine::userFactors() const {
  CHECK(userFactors_) << "user factors wasn't initialized";
  syncHost();
  return *userFactors_;
}

const FactorData& BPREngine::itemFactors() const {
  CHECK(itemFactors_) << "item factors wasn't initialized";
  syncHost();
  return *itemFactors_;
}

void BPREngine::saveUserFactors(const std::string& fileName) const {
  saveFactors(userFactors(), userIndex_, fileName);
}

void BPREngine::saveItemFactors(const std::string& fileName) const {
  saveFactors(itemFactors(), itemIndex_, fileName);
}

void BPREngine::saveUserRecommendations(const std::string& fileName, const size_t topN,
                                        const bool includeSeen,
                                        const std::vector<int64_t>* userIds,
                                        const RecommendScope& scope) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  CHECK_EQ(deviceOptions_.ngpus, 1) << "recommendations need --ngpus=1";
  saveRecommendations(dev_->get(), includeSeen ? QMFX_REC_ALL : QMFX_REC_UNSEEN_POSITIVES,
                      config_.useBiases, userIndex_, itemIndex_, fileName, topN, userIds, nullptr,
                      scope);
}

void BPREngine::saveItemSimilarities(const std::string& fileName, const size_t topN,
                                  const bool cosine, const std::vector<int64_t>* itemIds) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  saveSimilarities(dev_->get(), QMFX_ITEMS, itemIndex_, fileName, topN, cosine, itemIds);
}

void BPREngine::saveUserSimilarities(const std::string& fileName, const size_t topN,
                                  const bool cosine, const std::vector<int64_t>* userIds) const {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  saveSimilarities(dev_->get(), QMFX_USERS, userIndex_, fileName, topN, cosine, userIds);
}

size_t BPREngine::foldInUsers(const std::vector<DatasetElem>& lines,
                              const std::string& userFactorsFile,
                              const std::string& recommendationsFile, const size_t topN,
                              const bool includeSeen, const size_t epochs) {
  CHECK(dev_) << "no factor data, have you initialized the engine?";
  CHECK_GE(epochs, 1u) << "fold-in needs at least one epoch";
  if (!recommendationsFile.empty())
    CHECK(topN >= 1 && topN <= QMFX_REC_MAX_N)
        << "the number of recommendations must be in 1.." << QMFX_REC_MAX_N << ", got " << topN;
  // (user id, item idx) of the positive lines whose item the model knows
  std::vector<std::pair<int64_t, int32_t>> pairs;
  pairs.reserve(lines.size());
  size_t unknown = 0;
  for (const auto& e : lines) {
    if (e.value < 1.0) continue;
    const size_t i = itemIndex_.idx(e.itemId);
    if (i == IdIndex::missingIdx)
      ++unknown;
    else
      pairs.emplace_back(e.userId, static_cast<int32_t>(i));
  }
  if (unknown > 0)
    LOG(WARNING) << unknown << " fold-in lines name items that are not in the training data; dropped";
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  std::vector<int64_t> ids, rowptr(1, 0);
  std::vector<int32_t> col(pairs.size());
  for (size_t e = 0; e < pairs.size(); ++e) {
    if (e == 0 || pairs[e].first != pairs[e - 1].first) {
      if (e > 0) rowptr.push_back(static_cast<int64_t>(e));
      ids.push_back(pairs[e].first);
    }
    col[e] = pairs[e].second;
  }
  if (!pairs.empty()) rowptr.push_back(static_cast<int64_t>(pairs.size()));
  const size_t n = ids.size(), k = config_.nfactors;
  if (n == 0) {
    LOG(WARNING) << "no fold-in user has a positive on a known item; nothing folded in";
    if (!userFactorsFile.empty()) std::ofstream(userFactorsFile).flush();
    if (!recommendationsFile.empty()) std::ofstream(recommendationsFile).flush();
    return 0;
  }
  IdIndex index;
  index.assignSorted(std::move(ids));
  FactorData folded(n, k);
  qmfx_ctx* c = dev_->get();
  const uint64_t seed = (static_cast<uint64_t>(gen_()) << 32) | gen_();
  LOG(INFO) << "fold-in: " << n << " users, " << epochs << " epochs, sampling seed " << seed;
  const int numNeg = static_cast<int>(config_.numNegativeSamples);
  // optimize() decays the rate only below 1
  const Double decay = config_.decayRate < 1.0 ? config_.decayRate : 1.0;
  const int useBiases = config_.useBiases ? 1 : 0;
  if (recommendationsFile.empty()) {
    QMFX_CHECK(qmfx_bpr_fold_in(c, static_cast<int64_t>(n), rowptr.data(), col.data(), nullptr,
                                seed, static_cast<int>(epochs), numNeg, config_.initLearningRate,
                                decay, config_.userLambda, useBiases,
                                folded.getFactors().data(), nullptr));
  } else {
    std::vector<int64_t> items(n * topN), rows(n);
    std::vector<double> scores(n * topN);
    std::vector<int32_t> counts(n);
    for (size_t r = 0; r < n; ++r) rows[r] = static_cast<int64_t>(r);
    QMFX_CHECK(qmfx_bpr_recommend_fold_in(
        c, static_cast<int64_t>(n), rowptr.data(), col.data(), nullptr, seed,
        static_cast<int>(epochs), numNeg, config_.initLearningRate, decay, config_.userLambda,
        useBiases, static_cast<int>(topN), includeSeen ? 0 : 1, items.data(), scores.data(),
        counts.data(), folded.getFactors().data()));
    std::string text;
    formatPairs(index, itemIndex_, rows.data(), 0, n, topN, items.data(), scores.data(),
                counts.data(), text);
    std::ofstream fout(recommendationsFile);
    fout.write(text.data(), static_cast<std::streamsize>(text.size()));
  }
  if (!userFactorsFile.empty()) saveFactors(folded, index, userFactorsFile);
  return n;
}

}  // namespace qmf
