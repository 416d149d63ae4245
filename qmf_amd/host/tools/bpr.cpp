// `bpr` command line, drop-in for the reference's qmf/bpr.cpp:28-125: same flags, same log
// lines and output files.  Additions: --device, --precision (32 | 64), --seed (0 keeps the
// reference's random_device seeding), and the top-N recommendations of the trained model:
// --user_recommendations, --num_recommendations, --recommend_seen, --recommend_users, and one
// of --recommend_exclude_items, --recommend_items or --recommend_candidates (as in wals); and the
// items' / users' nearest neighbours in factor space: --item_similarities,
// --user_similarities, --num_similar, --similarity, --similar_item_ids, --similar_user_ids.
// New users (as in wals): --fold_in_dataset FILE ("user item weight" lines, the training format;
// its users are fitted by SGD against the trained item factors and biases, which stay as they
// are; lines with weight < 1 and lines naming an unknown item are dropped, the latter with a
// warning), --fold_in_user_factors OUT (the --user_factors format), --fold_in_recommendations
// OUT (the --user_recommendations format, honouring --num_recommendations and
// --recommend_seen) and --fold_in_epochs N (passes over a new user's items; default --nepochs).
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <memory>

#include <qmf/DatasetReader.h>
#include <qmf/bpr/BPREngine.h>
#include <qmf/metrics/MetricsEngine.h>
#include <qmf/utils/Flags.h>
#include <qmf/utils/Log.h>
#include <qmf/utils/Util.h>

// model arguments
DEFINE_uint64(nepochs, 10, "number of epochs for SGD");
DEFINE_uint64(nfactors, 30, "dimension of learned factors");
DEFINE_double(init_learning_rate, 0.05, "initial learning rate");
DEFINE_double(bias_lambda, 1.0, "regularization on biases");
DEFINE_double(user_lambda, 0.025, "regularization on user factors");
DEFINE_double(item_lambda, 0.0025, "regularization on item factors");
DEFINE_double(decay_rate, 0.9, "decay rate on learning rate");
DEFINE_bool(use_biases, false, "use bias term");
DEFINE_double(init_distribution_bound, 0.01, "init distirbution bound");
DEFINE_uint64(num_negative_samples, 3, "number of negative items to sample for each positive item");
DEFINE_uint64(num_hogwild_threads, 1,
              "accepted for compatibility: the device updates all positives in parallel");
DEFINE_bool(shuffle_training_set, true, "shuffle training set after each epoch");
// settings
DEFINE_uint64(eval_num_neg, 3, "number of negatives generated per positive in evaluation");
DEFINE_int32(eval_seed, 42, "random seed for generating evaluation set and test users");
DEFINE_uint64(nthreads, 16, "number of host threads (evaluation, output)");
DEFINE_int32(device, qmf::DeviceOptions::envInt("QMF_DEVICE", 0), "GPU ordinal");
DEFINE_int32(precision, qmf::DeviceOptions::envInt("QMF_PRECISION", 64),
             "device arithmetic: 64 (fp64, the reference's Double; default) or 32 (fp32)");
DEFINE_uint64(seed, 0, "seed of the factor init and SGD sampling (0 = random_device)");
// datasets
DEFINE_string(train_dataset, "", "filename of training dataset");
DEFINE_string(test_dataset, "", "filename of test dataset");
// metrics
DEFINE_string(test_avg_metrics, "", "comma-separated list of test metrics (averaged per-user)");
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

// new users
DEFINE_string(fold_in_dataset, "", "filename of new users' positives (the training format)");
DEFINE_string(fold_in_user_factors, "", "filename of the folded-in users' factors");
DEFINE_string(fold_in_recommendations, "",
              "filename of the folded-in users' top-N recommendations");
DEFINE_uint64(fold_in_epochs, 0, "SGD passes over a new user's items (0 = --nepochs)");

int main(int argc, char** argv) {
  if (!qmf::flags::parse(&argc, &argv, "bpr")) return 1;
  if (FLAGS_user_factors.empty() || FLAGS_item_factors.empty()) {
    LOG(WARNING) << "warning: missing model output filenames! (use options --{user,item}_factors)";
  }
  qmf::BPRConfig config{FLAGS_nepochs,
                        FLAGS_nfactors,
                        FLAGS_init_learning_rate,
                        FLAGS_bias_lambda,
                        FLAGS_user_lambda,
                        FLAGS_item_lambda,
                        FLAGS_decay_rate,
                        FLAGS_use_biases,
                        FLAGS_init_distribution_bound,
                        FLAGS_num_negative_samples,
                        FLAGS_num_hogwild_threads,
                        FLAGS_shuffle_training_set};
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
  CHECK(FLAGS_similarity == "cosine" || FLAGS_similarity == "dot")
      << "--similarity must be cosine or dot";
  if (!FLAGS_item_similarities.empty() || !FLAGS_user_similarities.empty())
    CHECK(FLAGS_num_similar >= 1 && FLAGS_num_similar <= QMFX_REC_MAX_N)
        << "--num_similar must be in 1.." << QMFX_REC_MAX_N;
  qmf::DeviceOptions device;
  device.device = FLAGS_device;
  device.precision = FLAGS_precision;
  qmf::BPREngine engine(config, metricsEngine, FLAGS_eval_num_neg, FLAGS_eval_seed,
                        FLAGS_nthreads, device);
  if (FLAGS_seed != 0) engine.seed(static_cast<uint32_t>(FLAGS_seed));

  LOG(INFO) << "loading training data";
  qmf::DatasetReader trainReader(FLAGS_train_dataset);
  engine.init(trainReader.readAll());
  if (!FLAGS_test_dataset.empty()) {
    LOG(INFO) << "loading test data";
    qmf::DatasetReader testReader(FLAGS_test_dataset);
    engine.initTest(testReader.readAll());
  }
  LOG(INFO) << "training";
  engine.optimize();
  if (!FLAGS_user_factors.empty() && !FLAGS_item_factors.empty()) {
    LOG(INFO) << "saving model output";
    engine.saveUserFactors(FLAGS_user_factors);
    engine.saveItemFactors(FLAGS_item_factors);
  }
  if (!FLAGS_user_recommendations.empty()) {
    LOG(INFO) << "saving recommendations";
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int64_t> ids;
    if (!FLAGS_recommend_users.empty()) ids = qmf::readIds(FLAGS_recommend_users);
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
    engine.saveUserRecommendations(FLAGS_user_recommendations, FLAGS_num_recommendations,
                                   FLAGS_recommend_seen,
                                   FLAGS_recommend_users.empty() ? nullptr : &ids, scope);
    // QMF_TIMINGS=1 (an addition, as in wals): the phase's wall time
    const char* tm = std::getenv("QMF_TIMINGS");
    if (tm && std::atoi(tm) > 0) {
      std::ifstream f(FLAGS_user_recommendations, std::ios::binary | std::ios::ate);
      LOG(INFO) << "timing: recommend "
                << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                << " s, " << (f ? static_cast<long long>(f.tellg()) : 0) << " bytes";
    }
  }
  if (!FLAGS_item_similarities.empty() || !FLAGS_user_similarities.empty()) {
    LOG(INFO) << "saving similarities";
    const auto t0 = std::chrono::steady_clock::now();
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
    const char* tm = std::getenv("QMF_TIMINGS");
    if (tm && std::atoi(tm) > 0)
      LOG(INFO) << "timing: similar "
                << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                << " s";
  }
  if (!FLAGS_fold_in_dataset.empty()) {
    LOG(INFO) << "folding in new users";
    const auto t0 = std::chrono::steady_clock::now();
    qmf::DatasetReader foldReader(FLAGS_fold_in_dataset);
    const size_t n = engine.foldInUsers(
        foldReader.readAll(), FLAGS_fold_in_user_factors, FLAGS_fold_in_recommendations,
        FLAGS_num_recommendations, FLAGS_recommend_seen,
        FLAGS_fold_in_epochs > 0 ? FLAGS_fold_in_epochs : FLAGS_nepochs);
    const char* tm = std::getenv("QMF_TIMINGS");
    if (tm && std::atoi(tm) > 0)
      LOG(INFO) << "timing: fold_in "
                << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
                << " s, " << n << " users";
  }
  return 0;
}
