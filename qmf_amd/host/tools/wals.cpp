// `wals` command line, drop-in for the reference's qmf/wals.cpp:26-107: same flags, same
// log lines and output files.  Additions: --device, --precision (32 | 64), --ngpus,
// --solver=exact|cg with --cg_steps (conjugate-gradient row solves, one GPU), and the
// top-N recommendations of the trained model: --user_recommendations, --num_recommendations,
// --recommend_seen, --recommend_users, and one of --recommend_exclude_items FILE (item ids never
// recommended), --recommend_items FILE (the only item ids recommended) or
// --recommend_candidates FILE ("user item weight" lines: these users, each only from the items
// listed with them); and the items' / users' nearest neighbours in factor space: --item_similarities, --user_similarities, --num_similar, --similarity,
// --similar_item_ids, --similar_user_ids; and fold-in of users the model was not trained on:
// --fold_in_dataset FILE ("user item weight" lines, the training format; its users are solved
// as new rows against the trained item factors even if their id was trained, and lines naming
// an unknown item are dropped with a warning), --fold_in_user_factors OUT (the --user_factors
// format) and --fold_in_recommendations OUT (the --user_recommendations format, honouring
// --num_recommendations and --recommend_seen); and why an item is recommended:
// --recommendation_explanations OUT (needs --user_recommendations) and --fold_in_explanations OUT
// (needs --fold_in_recommendations): for every (user, item) pair of the recommendations file,
// in its order, one line "<userId> <itemId> <sourceItemId> <contribution>" per source, the
// --num_explanations (default 5, 1..128) signals of the user that contribute most, in rank
// order.  A pair's contributions add up to the score of the user solved from the final item
// factors: the recommendation's score for a folded-in user, not for a trained one.
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <memory>

#include <qmf/DatasetReader.h>
#include <qmf/metrics/MetricsEngine.h>
#include <qmf/utils/Flags.h>
#include <qmf/utils/Log.h>
#include <qmf/utils/Util.h>
#include <qmf/wals/WALSEngine.h>

// model arguments
DEFINE_uint64(nepochs, 10, "number of epochs for ALS");
DEFINE_uint64(nfactors, 30, "dimension of learned factors");
DEFINE_double(regularization_lambda, 0.05, "regularization param");
DEFINE_double(confidence_weight, 40, "confidence weight");
DEFINE_double(init_distribution_bound, 0.01, "init distirbution bound");
DEFINE_string(distribution_file, "", "uniform distribution file, for repeatable result");
DEFINE_string(solver, "exact",
              "row solves: exact (factorization, the reference's) or cg (--cg_steps warm-started "
              "conjugate-gradient steps per row and half; one GPU)");
DEFINE_int32(cg_steps, 3, "conjugate-gradient steps per row and half with --solver=cg");
// settings
DEFINE_int32(nthreads, 16, "number of host threads (ingest, evaluation, output)");
DEFINE_int32(device, qmf::DeviceOptions::envInt("QMF_DEVICE", 0), "GPU ordinal");
DEFINE_int32(precision, qmf::DeviceOptions::envInt("QMF_PRECISION", 64),
             "device arithmetic: 64 (fp64, the reference's Double; default) or 32 (fp32)");
DEFINE_int32(ngpus, qmf::DeviceOptions::envInt("QMF_NGPUS", 1),
             "GPUs to split the rows over (devices --device .. --device+ngpus-1, RCCL "
             "all-gather per half-epoch)");
// datasets
DEFINE_string(train_dataset, "", "filename of training dataset");
DEFINE_string(test_dataset, "", "filename of test dataset");
// metrics
DEFINE_string(test_avg_metrics, "", "comma-separated list of test metrics (averaged per-user)");
DEFINE_int32(eval_seed, 42, "random seed for picking test users");
DEFINE_uint64(num_test_users, 0, "# users to use for computing test avg metrics (0 = all users)");
DEFINE_bool(test_always, false,
            "whether to compute test avg metrics after each epoch (if false, only computes at "
            "the end)");
// model output
DEFINE_string(user_factors, "", "filename of user factors");
DEFINE_string(item_factors, "", "filename of item factors");
// recommendations
DEFINE_string(user_recommendations, "", "filename of the users' top-N recommendations");
DEFINE_uint64(num_recommendations, 10, "items recommended per user (1..128)");
DEFINE_bool(recommend_seen, false, "also recommend items of the user's training data");
DEFINE_bool(recommend_screen, false,
            "select --user_recommendations through the f32 screen and exact re-rank "
            "(qmfx_recommend_screened): the same file, faster on large catalogues");
DEFINE_string(recommend_users, "",
              "file with one user id per line to recommend for (default: every training user)");
DEFINE_string(recommend_exclude_items, "",
              "file with one item id per line that is never recommended");
DEFINE_string(recommend_items, "",
              "file with one item id per line: recommendations come only from these items");
DEFINE_string(recommend_candidates, "",
              "file of 'user item weight' lines (the training format, the weight is ignored): "
              "recommend to exactly these users, each only from the items listed with them");
// similar items / users (nearest neighbours in factor space)
DEFINE_string(item_similarities, "", "filename of the items' top-N most similar items");
DEFINE_string(user_similarities, "", "filename of the users' top-N most similar users");
DEFINE_uint64(num_similar, 10, "neighbours listed per item or user (1..128)");
DEFINE_string(similarity, "cosine", "similarity of two factor rows: cosine or dot");
DEFINE_string(similar_item_ids, "",
              "file with one item id per line to list neighbours for (default: every item)");
DEFINE_string(similar_user_ids, "",
              "file with one user id per line to list neighbours for (default: every user)");

// fold-in of new users
DEFINE_string(fold_in_dataset, "", "filename of new users' signals (the training format)");
DEFINE_string(fold_in_user_factors, "", "filename of the folded-in users' factors");
DEFINE_string(fold_in_recommendations, "",
              "filename of the folded-in users' top-N recommendations");
// explanations
DEFINE_string(recommendation_explanations, "",
              "filename of the per-signal contributions to the pairs of --user_recommendations");
DEFINE_string(fold_in_explanations, "",
              "filename of the per-signal contributions to the pairs of --fold_in_recommendations");
DEFINE_uint64(num_explanations, 5, "sources listed per recommended pair (1..128)");

namespace {
// QMF_TIMINGS=1 (an addition; unset, the output is the reference's): one "timing:" log line per
// phase with its wall time, read by tools/bench_cli.py
bool timings() {
  static const bool on = std::getenv("QMF_TIMINGS") && std::atoi(std::getenv("QMF_TIMINGS")) > 0;
  return on;
}
double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
long long fileBytes(const std::string& f) {
  std::ifstream s(f, std::ios::binary | std::ios::ate);
  return s ? static_cast<long long>(s.tellg()) : 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (!qmf::flags::parse(&argc, &argv, "wals")) return 1;
  if (FLAGS_user_factors.empty() || FLAGS_item_factors.empty()) {
    LOG(WARNING) << "warning: missing model output filenames! (use options --{user,item}_factors)";
  }
  CHECK(FLAGS_solver == "exact" || FLAGS_solver == "cg") << "--solver must be exact or cg";
  CHECK(FLAGS_cg_steps >= 1) << "--cg_steps must be at least 1";
  CHECK(FLAGS_solver != "cg" || FLAGS_ngpus <= 1) << "--solver=cg runs on one GPU (--ngpus 1)";
  qmf::WALSConfig config{FLAGS_nepochs,
                         FLAGS_nfactors,
                         FLAGS_regularization_lambda,
                         FLAGS_confidence_weight,
                         FLAGS_init_distribution_bound,
                         FLAGS_distribution_file,
                         FLAGS_solver == "cg" ? static_cast<size_t>(FLAGS_cg_steps) : 0};
  qmf::MetricsConfig metricsConfig{FLAGS_num_test_users, FLAGS_test_always, FLAGS_eval_seed};
  const auto metricsEngine = std::make_unique<qmf::MetricsEngine>(metricsConfig);
  for (const auto& metric : qmf::split(FLAGS_test_avg_metrics, ',')) {
    CHECK(metricsEngine->addTestAvgMetric(metric)) << "metric " << metric << " is not available";
  }
  if (!FLAGS_fold_in_user_factors.empty() || !FLAGS_fold_in_recommendations.empty())
    CHECK(!FLAGS_fold_in_dataset.empty())
        << "--fold_in_user_factors and --fold_in_recommendations need --fold_in_dataset";
  if (!FLAGS_user_recommendations.empty() || !FLAGS_fold_in_recommendations.empty())
    CHECK(FLAGS_num_recommendations >= 1 && FLAGS_num_recommendations <= QMFX_REC_MAX_N)
        << "--num_recommendations must be in 1.." << QMFX_REC_MAX_N;
  {
    // what may be recommended: at most one of the three scope flags, on --user_recommendations
    const int scopes = !FLAGS_recommend_exclude_items.empty() + !FLAGS_recommend_items.empty() +
                       !FLAGS_recommend_candidates.empty();
    CHECK(!FLAGS_recommend_screen || scopes == 0)
        << "--recommend_screen scans the whole catalogue: it does not combine with "
           "--recommend_exclude_items, --recommend_items or --recommend_candidates";
    CHECK(scopes <= 1) << "--recommend_exclude_items, --recommend_items and "
                          "--recommend_candidates are mutually exclusive";
    CHECK(FLAGS_recommend_candidates.empty() || FLAGS_recommend_users.empty())
        << "--recommend_candidates and --recommend_users are mutually exclusive";
    CHECK(scopes == 0 || !FLAGS_user_recommendations.empty())
        << "--recommend_exclude_items, --recommend_items and --recommend_candidates need "
           "--user_recommendations";
  }
  if (!FLAGS_recommendation_explanations.empty())
    CHECK(!FLAGS_user_recommendations.empty())
        << "--recommendation_explanations needs --user_recommendations";
  if (!FLAGS_fold_in_explanations.empty())
    CHECK(!FLAGS_fold_in_recommendations.empty())
        << "--fold_in_explanations needs --fold_in_recommendations";
  if (!FLAGS_recommendation_explanations.empty() || !FLAGS_fold_in_explanations.empty())
    CHECK(FLAGS_num_explanations >= 1 && FLAGS_num_explanations <= QMFX_REC_MAX_N)
        << "--num_explanations must be in 1.." << QMFX_REC_MAX_N;
  CHECK(FLAGS_similarity == "cosine" || FLAGS_similarity == "dot")
      << "--similarity must be cosine or dot";
  if (!FLAGS_item_similarities.empty() || !FLAGS_user_similarities.empty())
    CHECK(FLAGS_num_similar >= 1 && FLAGS_num_similar <= QMFX_REC_MAX_N)
        << "--num_similar must be in 1.." << QMFX_REC_MAX_N;
  qmf::DeviceOptions device;
  device.device = FLAGS_device;
  device.precision = FLAGS_precision;
  device.ngpus = FLAGS_ngpus;
  qmf::WALSEngine engine(config, metricsEngine, static_cast<size_t>(FLAGS_nthreads), device);

  LOG(INFO) << "loading training data";
  double t0 = now();
  qmf::DatasetReader trainReader(FLAGS_train_dataset);
  {
    const auto data = trainReader.readAll();
    const double t1 = now();
    if (timings())
      LOG(INFO) << "timing: parse " << t1 - t0 << " s, " << fileBytes(FLAGS_train_dataset)
                << " bytes, " << data.size() << " lines";
    engine.init(data);
    if (timings()) LOG(INFO) << "timing: init " << now() - t1 << " s";
  }
  if (!FLAGS_test_dataset.empty()) {
    LOG(INFO) << "loading test data";
    qmf::DatasetReader testReader(FLAGS_test_dataset);
    engine.initTest(testReader.readAll());
  }
  LOG(INFO) << "training";
  t0 = now();
  engine.optimize();
  if (timings()) LOG(INFO) << "timing: optimize " << now() - t0 << " s, " << FLAGS_nepochs << " epochs";
  if (!FLAGS_user_factors.empty() && !FLAGS_item_factors.empty()) {
    LOG(INFO) << "saving model output";
    t0 = now();
    engine.saveUserFactors(FLAGS_user_factors);
    engine.saveItemFactors(FLAGS_item_factors);
    if (timings())
      LOG(INFO) << "timing: save " << now() - t0 << " s, "
                << fileBytes(FLAGS_user_factors) + fileBytes(FLAGS_item_factors) << " bytes";
  }
  if (!FLAGS_user_recommendations.empty()) {
    LOG(INFO) << "saving recommendations";
    t0 = now();
    std::vector<int64_t> ids;
    if (!FLAGS_recommend_users.empty()) ids = qmf::readIds(FLAGS_recommend_users);
    const std::vector<int64_t>* users = FLAGS_recommend_users.empty() ? nullptr : &ids;
    // the scope flags' files, read into the scope of the save call
    std::vector<int64_t> scopeIds;
    std::vector<qmf::DatasetElem> scopeLines;
    qmf::RecommendScope scope;
    scope.screen = FLAGS_recommend_screen;
    if (!FLAGS_recommend_exclude_items.empty()) {
      scopeIds = qmf::readIds(FLAGS_recommend_exclude_items);
      scope.excludeItemIds = &scopeIds;
    } else if (!FLAGS_recommend_items.empty()) {
      scopeIds = qmf::readIds(FLAGS_recommend_items);
      scope.itemIds = &scopeIds;
    } else if (!FLAGS_recommend_candidates.empty()) {
      qmf::DatasetReader candReader(FLAGS_recommend_candidates);
      scopeLines = candReader.readAll();
      scope.candidates = &scopeLines;
    }
    if (FLAGS_recommendation_explanations.empty())
      engine.saveUserRecommendations(FLAGS_user_recommendations, FLAGS_num_recommendations,
                                     FLAGS_recommend_seen, users, scope);
    else
      engine.saveRecommendationExplanations(
          FLAGS_user_recommendations, FLAGS_recommendation_explanations,
          FLAGS_num_recommendations, FLAGS_num_explanations, FLAGS_recommend_seen, users, scope);
    if (timings())
      LOG(INFO) << "timing: recommend " << now() - t0 << " s, "
                << fileBytes(FLAGS_user_recommendations) << " bytes";
  }
  if (!FLAGS_item_similarities.empty() || !FLAGS_user_similarities.empty()) {
    LOG(INFO) << "saving similarities";
    t0 = now();
    const bool cosine = FLAGS_similarity == "cosine";
    std::vector<int64_t> ids;
    if (!FLAGS_item_similarities.empty()) {
      if (!FLAGS_similar_item_ids.empty()) ids = qmf::readIds(FLAGS_similar_item_ids);
      engine.saveItemSimilarities(FLAGS_item_similarities, FLAGS_num_similar, cosine,
                                  FLAGS_similar_item_ids.empty() ? nullptr : &ids);
    }
    if (!FLAGS_user_similarities.empty()) {
      if (!FLAGS_similar_user_ids.empty()) ids = qmf::readIds(FLAGS_similar_user_ids);
      engine.saveUserSimilarities(FLAGS_user_similarities, FLAGS_num_similar, cosine,
                                  FLAGS_similar_user_ids.empty() ? nullptr : &ids);
    }
    if (timings())
      LOG(INFO) << "timing: similar " << now() - t0 << " s, "
                << fileBytes(FLAGS_item_similarities) + fileBytes(FLAGS_user_similarities)
                << " bytes";
  }
  if (!FLAGS_fold_in_dataset.empty()) {
    LOG(INFO) << "folding in new users";
    t0 = now();
    qmf::DatasetReader foldReader(FLAGS_fold_in_dataset);
    const size_t n = engine.foldInUsers(foldReader.readAll(), FLAGS_fold_in_user_factors,
                                        FLAGS_fold_in_recommendations,
                                        FLAGS_num_recommendations, FLAGS_recommend_seen,
                                        FLAGS_fold_in_explanations, FLAGS_num_explanations);
    if (timings())
      LOG(INFO) << "timing: fold_in " << now() - t0 << " s, " << n << " users, "
                << fileBytes(FLAGS_fold_in_user_factors) + fileBytes(FLAGS_fold_in_recommendations)
                << " bytes";
  }
  return 0;
}
