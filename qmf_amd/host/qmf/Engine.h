// Base class of the drop-in engines (reference: qmf/Engine.h:32-96, Engine.cpp:27-122).
// Non-copyable, non-movable; errors abort through CHECK as in the reference.
#pragma once

#include <functional>
#include <ostream>
#include <string>
#include <vector>

#include <qmf/DatasetReader.h>
#include <qmf/FactorData.h>
#include <qmf/metrics/Metrics.h>
#include <qmf/Types.h>
#include <qmf/utils/IdIndex.h>
#include <qmf/utils/ParallelExecutor.h>
#include <qmfx.h>

namespace qmf {

// Which items a saveUserRecommendations call may recommend; at most one member is set (none:
// every item).  Ids the model does not know are skipped with one warning carrying their count.
struct RecommendScope {
  // item ids that are never recommended (include/qmfx.h qmfx_recommend_without)
  const std::vector<int64_t>* excludeItemIds = nullptr;
  // the only item ids that are recommended, to every user (qmfx_recommend_candidates, shared list)
  const std::vector<int64_t>* itemIds = nullptr;
  // per-user candidates as dataset lines (the value is ignored): a user is recommended only the
  // items listed with them, and the requested users are exactly the lines' known users, in
  // ascending user idx; excludes userIds
  const std::vector<DatasetElem>* candidates = nullptr;
  // not a narrower scope but another route to the same lists: the whole catalogue through
  // qmfx_recommend_screened (an f32 screen, then an exact re-rank; the file is byte for byte
  // the one written without it).  Only without a list above.
  bool screen = false;
};

class Engine {
 public:
  Engine() = default;
  virtual ~Engine() = default;
  Engine(const Engine&) = delete;
  Engine(Engine&&) = delete;
  Engine& operator=(const Engine&) = delete;
  Engine& operator=(Engine&&) = delete;

  virtual void init(const std::vector<DatasetElem>& dataset) {}
  virtual void initTest(const std::vector<DatasetElem>& testDataset) {}
  virtual void optimize() {}
  virtual void evaluate(const size_t epoch) {}
  virtual void saveUserFactors(const std::string& fileName) const {}
  virtual void saveItemFactors(const std::string& fileName) const {}
  // Addition to the reference API: the topN (1..QMFX_REC_MAX_N) best items of every training
  // user (ascending user idx), or of the users in `userIds` in that order (unknown ids are
  // skipped with one warning), selected on the device from the current factors.  One line
  // "<userId> <itemId> <score>\n" per pair, scores with 9 decimals, each user's lines in rank
  // order (higher score first, equal scores by ascending item idx): the dataset format, so
  // DatasetReader reads the file back.  includeSeen = false leaves the user's training items
  // out; a user with no eligible item writes nothing.  `scope` narrows the eligible items.
  virtual void saveUserRecommendations(const std::string& fileName, size_t topN, bool includeSeen,
                                       const std::vector<int64_t>* userIds = nullptr,
                                       const RecommendScope& scope = RecommendScope()) const {}
  // Addition to the reference API: the topN (1..QMFX_REC_MAX_N) nearest items of every item
  // (ascending item idx), or of the items in `itemIds` in that order (unknown ids are skipped
  // with one warning), among the items, by cosine (else by dot product) of the current factors,
  // selected on the device (include/qmfx.h qmfx_similar).  One line "<id> <neighbourId>
  // <score>\n" per pair, scores with 9 decimals, each query's lines in rank order (higher
  // score first, equal scores by ascending idx): the dataset format.  The query itself is
  // always left out.  saveUserSimilarities: the same for users among the users.
  virtual void saveItemSimilarities(const std::string& fileName, size_t topN, bool cosine,
                                    const std::vector<int64_t>* itemIds = nullptr) const {}
  virtual void saveUserSimilarities(const std::string& fileName, size_t topN, bool cosine,
                                    const std::vector<int64_t>* userIds = nullptr) const {}

  // The query rows of a save call: the idx of every id of `ids` that `index` knows, in that
  // order (the others are skipped with one warning carrying their count, `what` naming them),
  // or every idx ascending when ids is null.
  static std::vector<int64_t> queryRows(const IdIndex& index, const std::vector<int64_t>* ids,
                                        const char* what);

  // Appends "<queryId> <otherId> <score>\n" (%.9f) for queries [b, e) of a batch: query t is
  // idx rows[t] of queryIndex and lists others[t·topN + r] (idx of otherIndex) with
  // scores[t·topN + r] for r < counts[t].
  static void formatPairs(const IdIndex& queryIndex, const IdIndex& otherIndex,
                          const int64_t* rows, size_t b, size_t e, size_t topN,
                          const int64_t* others, const double* scores, const int32_t* counts,
                          std::string& s);

  // Appends "<queryId> <targetId> <sourceId> <contribution>\n" (%.9f) for pairs [b, e): pair p
  // is query idx pairRows[p] of queryIndex and target idx targets[p] of otherIndex, explained
  // by sources[p·topM + s] (idx of otherIndex) with contribs[p·topM + s] for s < counts[p].
  static void formatExplanations(const IdIndex& queryIndex, const IdIndex& otherIndex,
                                 const int64_t* pairRows, const int64_t* targets, size_t b,
                                 size_t e, size_t topM, const int64_t* sources,
                                 const double* contribs, const int32_t* counts, std::string& s);

  // called after a batch of a save call has been selected: its n query rows and their lists
  using AfterBatch = std::function<void(const int64_t* rows, size_t n, const int64_t* others,
                                        const int32_t* counts)>;

 protected:
  // saveUserRecommendations of the engines: qmfx_recommend (include/qmfx.h) with the given
  // exclude mode in batches of at most 65,536 users, formatted and written batch by batch;
  // `after` (unless null) sees every batch's lists once they are selected.  With a scope the
  // batches go to qmfx_recommend_without / qmfx_recommend_candidates, the item lists sorted and
  // deduplicated here.
  static void saveRecommendations(qmfx_ctx* ctx, int exclude, bool useBiases,
                                  const IdIndex& userIndex, const IdIndex& itemIndex,
                                  const std::string& fileName, size_t topN,
                                  const std::vector<int64_t>* userIds,
                                  const AfterBatch* after = nullptr,
                                  const RecommendScope& scope = RecommendScope());

  // formatExplanations of all the pairs, in blocks in parallel, written to `out` in order
  static void writeExplanations(const IdIndex& queryIndex, const IdIndex& otherIndex,
                                const std::vector<int64_t>& pairRows,
                                const std::vector<int64_t>& targets, size_t topM,
                                const int64_t* sources, const double* contribs,
                                const int32_t* counts, std::ostream& out);

  // save{Item,User}Similarities of the engines: qmfx_similar on `side` (whose id table is
  // `index`) in batches of at most 65,536 queries, written batch by batch
  static void saveSimilarities(qmfx_ctx* ctx, int side, const IdIndex& index,
                               const std::string& fileName, size_t topN, bool cosine,
                               const std::vector<int64_t>* ids);

  // test users (those with at least one known (user, item) test pair), optionally a
  // sample of numTestUsers of them shuffled with mt19937(seed), and their dense label rows
  static void initAvgTestData(std::vector<size_t>& testUsers,
                              std::vector<std::vector<Double>>& testLabels,
                              std::vector<std::vector<Double>>& testScores,
                              const std::vector<DatasetElem>& testDataset,
                              const IdIndex& userIndex,
                              const IdIndex& itemIndex,
                              const size_t numTestUsers = 0,
                              const int32_t seed = 0);

  // scores[u][i] = bias_i + <user_u, item_i> for every test user and item
  static void computeTestScores(std::vector<std::vector<Double>>& testScores,
                                const std::vector<size_t>& testUsers,
                                const FactorData& userFactors,
                                const FactorData& itemFactors,
                                ParallelExecutor& parallel);

  // Device evaluation (addition to the reference API): the same per-user metrics without the
  // dense score matrix.  The non-zero test labels go to the device once (as a CSR over the
  // test users); each call scores the context's current factors there and returns one
  // RankedUser per test user (include/qmfx.h qmfx_eval_ranks).
  void computeTestRanks(qmfx_ctx* ctx, bool useBiases, const std::vector<size_t>& testUsers,
                        const std::vector<std::vector<Double>>& testLabels,
                        std::vector<RankedUser>& ranks);

  // "<id>[ <bias>] <f0> ... <fk-1>\n" per idx, std::fixed with 9 decimals
  static void saveFactors(const FactorData& factorData, const IdIndex& index,
                          const std::string& fileName);
  static void saveFactors(const FactorData& factorData, const IdIndex& index, std::ostream& out);

  friend class EngineTestPeer;

 private:
  struct TestLabelCsr {
    std::vector<int64_t> rowptr, items;
    std::vector<Double> values;
    size_t npos = 0;
    bool uploaded = false;
  } testCsr_;
};

}  // namespace qmf
