#include <qmf/Engine.h>

#include <charconv>

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <random>
#include <thread>
#include <unordered_map>
#include <unordered_set>

#include <qmf/Device.h>
#include <qmf/utils/Log.h>

namespace qmf {

void Engine::initAvgTestData(std::vector<size_t>& testUsers,
                             std::vector<std::vector<Double>>& testLabels,
                             std::vector<std::vector<Double>>& testScores,
                             const std::vector<DatasetElem>& testDataset,
                             const IdIndex& userIndex,
                             const IdIndex& itemIndex,
                             const size_t numTestUsers,
                             const int32_t seed) {
  // The user order is the iteration order of an unordered_set filled in dataset order,
  // then (optionally) a mt19937(seed) shuffle: the same containers and calls as the
  // reference (Engine.cpp:35-52) so the sampled users coincide.
  std::unordered_set<size_t> seen;
  for (const auto& e : testDataset) {
    const size_t u = userIndex.idx(e.userId);
    const size_t i = itemIndex.idx(e.itemId);
    if (u != IdIndex::missingIdx && i != IdIndex::missingIdx) seen.insert(u);
  }
  testUsers.assign(seen.begin(), seen.end());
  if (numTestUsers > 0 && numTestUsers < testUsers.size()) {
    std::shuffle(testUsers.begin(), testUsers.end(), std::mt19937(seed));
    testUsers.resize(numTestUsers);
    testUsers.shrink_to_fit();
  }
  std::unordered_map<size_t, size_t> slot;
  testLabels.reserve(testUsers.size());
  testScores.reserve(testUsers.size());
  for (size_t t = 0; t < testUsers.size(); ++t) {
    slot[testUsers[t]] = t;
    testLabels.emplace_back(itemIndex.size());
    testScores.emplace_back(itemIndex.size());
  }
  for (const auto& e : testDataset) {
    const size_t u = userIndex.idx(e.userId);
    const size_t i = itemIndex.idx(e.itemId);
    if (u == IdIndex::missingIdx || i == IdIndex::missingIdx) continue;
    const auto it = slot.find(u);
    if (it != slot.end()) testLabels[it->second][i] = e.value;
  }
}

void Engine::computeTestScores(std::vector<std::vector<Double>>& testScores,
                               const std::vector<size_t>& testUsers,
                               const FactorData& userFactors,
                               const FactorData& itemFactors,
                               ParallelExecutor& parallel) {
  const size_t k = userFactors.nfactors();
  const size_t ni = itemFactors.nelems();
  parallel.execute(testUsers.size(), [&](const size_t t) {
    const Double* u = userFactors.getFactors().data(testUsers[t]);
    auto& scores = testScores[t];
    for (size_t i = 0; i < ni; ++i) {
      const Double* q = itemFactors.getFactors().data(i);
      Double s = itemFactors.withBiases() ? itemFactors.biasAt(i) : 0.0;
      for (size_t f = 0; f < k; ++f) s += u[f] * q[f];
      scores[i] = s;
    }
  });
}

void Engine::computeTestRanks(qmfx_ctx* ctx, bool useBiases,
                              const std::vector<size_t>& testUsers,
                              const std::vector<std::vector<Double>>& testLabels,
                              std::vector<RankedUser>& ranks) {
  CHECK_EQ(testUsers.size(), testLabels.size());
  const size_t nt = testUsers.size();
  auto& L = testCsr_;
  if (!L.uploaded) {
    L.rowptr.assign(1, 0);
    for (const auto& row : testLabels) {
      for (size_t i = 0; i < row.size(); ++i)
        if (row[i] != 0.0) {
          L.items.push_back(static_cast<int64_t>(i));
          L.values.push_back(row[i]);
          L.npos += row[i] > 0.0;
        }
      L.rowptr.push_back(static_cast<int64_t>(L.items.size()));
    }
    const std::vector<int64_t> users(testUsers.begin(), testUsers.end());
    QMFX_CHECK(qmfx_eval_set_labels(ctx, static_cast<int64_t>(nt), users.data(),
                                    L.rowptr.data(), L.items.data(), L.values.data()));
    L.uploaded = true;
  }
  std::vector<double> lscore(L.items.size()), sq(nt);
  std::vector<int64_t> above(L.npos);
  QMFX_CHECK(qmfx_eval_ranks(ctx, useBiases ? 1 : 0, lscore.data(), above.data(), sq.data()));
  ranks.assign(nt, RankedUser());
  size_t p = 0;
  for (size_t t = 0; t < nt; ++t) {
    RankedUser& r = ranks[t];
    r.nitems = testLabels[t].size();
    // Σ score² over all items, with the labelled items' terms swapped for (label − score)²
    Double sse = sq[t];
    std::vector<Double> ps;
    std::vector<int64_t> ab;
    for (int64_t e = L.rowptr[t]; e < L.rowptr[t + 1]; ++e) {
      const Double l = L.values[e], s = lscore[e];
      sse += (l - s) * (l - s) - s * s;
      if (l > 0.0) {
        ps.push_back(s);
        ab.push_back(above[p++]);
      }
    }
    r.sse = sse;
    r.setPositives(ps, ab);
  }
}

namespace {

// " %.9f" of x appended to s.  std::to_chars with a precision renders the exact decimal value
// of x correctly rounded, as glibc's printf does, so the text is the same byte for byte (the
// host tests compare them over random and edge values); a value that does not fit the buffer
// (|x| ≥ 1e290) takes printf itself.
inline void appendFixed9(std::string& s, Double x) {
  char buf[320];
  buf[0] = ' ';
  const auto r = std::to_chars(buf + 1, buf + sizeof(buf), x, std::chars_format::fixed, 9);
  if (r.ec == std::errc()) {
    s.append(buf, r.ptr);
    return;
  }
  std::string big(static_cast<size_t>(std::snprintf(nullptr, 0, " %.9f", x)) + 1, '\0');
  std::snprintf(&big[0], big.size(), " %.9f", x);
  big.pop_back();
  s += big;
}

// Formats rows [b, e) exactly as `out << std::fixed << std::setprecision(9)` would:
// libstdc++ renders fixed doubles through printf("%.*f").
void formatRows(const FactorData& fd, const IdIndex& index, size_t b, size_t e, std::string& s) {
  char buf[32];
  const size_t k = fd.nfactors();
  s.reserve(s.size() + (e - b) * (k * 13 + 24));
  for (size_t idx = b; idx < e; ++idx) {
    s.append(buf, std::to_chars(buf, buf + sizeof(buf), static_cast<long long>(index.id(idx))).ptr);
    if (fd.withBiases()) appendFixed9(s, fd.biasAt(idx));
    const Double* row = fd.getFactors().data(idx);
    for (size_t f = 0; f < k; ++f) appendFixed9(s, row[f]);
    s.push_back('\n');
  }
}

}  // namespace

void Engine::saveFactors(const FactorData& factorData, const IdIndex& index,
                         const std::string& fileName) {
  std::ofstream fout(fileName);
  saveFactors(factorData, index, fout);
}

std::vector<int64_t> Engine::queryRows(const IdIndex& index, const std::vector<int64_t>* ids,
                                       const char* what) {
  std::vector<int64_t> rows;
  if (ids) {
    size_t unknown = 0;
    for (const int64_t id : *ids) {
      const size_t r = index.idx(id);
      if (r == IdIndex::missingIdx)
        ++unknown;
      else
        rows.push_back(static_cast<int64_t>(r));
    }
    if (unknown > 0)
      LOG(WARNING) << unknown << " requested " << what
                   << " ids are not in the training data; skipped";
  } else {
    rows.resize(index.size());
    for (size_t r = 0; r < rows.size(); ++r) rows[r] = static_cast<int64_t>(r);
  }
  return rows;
}

void Engine::formatPairs(const IdIndex& queryIndex, const IdIndex& otherIndex,
                         const int64_t* rows, const size_t b, const size_t e, const size_t topN,
                         const int64_t* others, const double* scores, const int32_t* counts,
                         std::string& s) {
  char buf[32];
  for (size_t t = b; t < e; ++t) {
    const long long qid = static_cast<long long>(queryIndex.id(static_cast<size_t>(rows[t])));
    for (int32_t r = 0; r < counts[t]; ++r) {
      s.append(buf, std::to_chars(buf, buf + sizeof(buf), qid).ptr);
      s.push_back(' ');
      const size_t other = static_cast<size_t>(others[t * topN + r]);
      s.append(buf, std::to_chars(buf, buf + sizeof(buf),
                                  static_cast<long long>(otherIndex.id(other))).ptr);
      appendFixed9(s, scores[t * topN + r]);
      s.push_back('\n');
    }
  }
}

void Engine::formatExplanations(const IdIndex& queryIndex, const IdIndex& otherIndex,
                                const int64_t* pairRows, const int64_t* targets, const size_t b,
                                const size_t e, const size_t topM, const int64_t* sources,
                                const double* contribs, const int32_t* counts, std::string& s) {
  char buf[32];
  for (size_t p = b; p < e; ++p) {
    std::string head;
    head.append(buf, std::to_chars(buf, buf + sizeof(buf), static_cast<long long>(queryIndex.id(
                                                               static_cast<size_t>(pairRows[p])))).ptr);
    head.push_back(' ');
    head.append(buf, std::to_chars(buf, buf + sizeof(buf), static_cast<long long>(otherIndex.id(
                                                               static_cast<size_t>(targets[p])))).ptr);
    head.push_back(' ');
    for (int32_t r = 0; r < counts[p]; ++r) {
      s += head;
      const size_t src = static_cast<size_t>(sources[p * topM + r]);
      s.append(buf, std::to_chars(buf, buf + sizeof(buf),
                                  static_cast<long long>(otherIndex.id(src))).ptr);
      appendFixed9(s, contribs[p * topM + r]);
      s.push_back('\n');
    }
  }
}

void Engine::writeExplanations(const IdIndex& queryIndex, const IdIndex& otherIndex,
                               const std::vector<int64_t>& pairRows,
                               const std::vector<int64_t>& targets, const size_t topM,
                               const int64_t* sources, const double* contribs,
                               const int32_t* counts, std::ostream& out) {
  const size_t n = targets.size(), block = 4096, nblocks = (n + block - 1) / block;
  const unsigned hc = std::thread::hardware_concurrency();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(hc ? hc : 1, 16));
  for (size_t b0 = 0; b0 < nblocks; b0 += nt) {
    const size_t nb = std::min(nt, nblocks - b0);
    std::vector<std::string> parts(nb);
    ParallelExecutor::run(nb, [&](const size_t p) {
      const size_t b = (b0 + p) * block, e = std::min(n, b + block);
      formatExplanations(queryIndex, otherIndex, pairRows.data(), targets.data(), b, e, topM,
                         sources, contribs, counts, parts[p]);
    });
    for (const auto& p : parts) out.write(p.data(), static_cast<std::streamsize>(p.size()));
  }
}

namespace {

// The batches of a save call: `select` fills one batch's lists (n queries from rows + r0),
// which are formatted in blocks in parallel and written in order.
template <typename Select>
void savePairs(const IdIndex& queryIndex, const IdIndex& otherIndex,
               const std::vector<int64_t>& rows, const std::string& fileName, const size_t topN,
               const Select& select, const Engine::AfterBatch* after = nullptr) {
  std::ofstream fout(fileName);
  const size_t batch = 65536, block = 4096;
  const unsigned hc = std::thread::hardware_concurrency();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(hc ? hc : 1, batch / block));
  std::vector<int64_t> others(std::min(batch, rows.size()) * topN);
  std::vector<double> scores(others.size());
  std::vector<int32_t> counts(std::min(batch, rows.size()));
  for (size_t r0 = 0; r0 < rows.size(); r0 += batch) {
    const size_t n = std::min(batch, rows.size() - r0);
    select(rows.data() + r0, n, others.data(), scores.data(), counts.data());
    if (after) (*after)(rows.data() + r0, n, others.data(), counts.data());
    const size_t nblocks = (n + block - 1) / block;
    for (size_t b0 = 0; b0 < nblocks; b0 += nt) {
      const size_t nb = std::min(nt, nblocks - b0);
      std::vector<std::string> parts(nb);
      ParallelExecutor::run(nb, [&](const size_t p) {
        const size_t b = (b0 + p) * block, e = std::min(n, b + block);
        Engine::formatPairs(queryIndex, otherIndex, rows.data() + r0, b, e, topN, others.data(),
                            scores.data(), counts.data(), parts[p]);
      });
      for (const auto& p : parts) fout.write(p.data(), static_cast<std::streamsize>(p.size()));
    }
  }
}

}  // namespace

namespace {

std::vector<int64_t> sortedUnique(std::vector<int64_t> v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

}  // namespace

void Engine::saveRecommendations(qmfx_ctx* ctx, const int exclude, const bool useBiases,
                                 const IdIndex& userIndex, const IdIndex& itemIndex,
                                 const std::string& fileName, const size_t topN,
                                 const std::vector<int64_t>* userIds, const AfterBatch* after,
                                 const RecommendScope& scope) {
  CHECK(topN >= 1 && topN <= QMFX_REC_MAX_N)
      << "the number of recommendations must be in 1.." << QMFX_REC_MAX_N << ", got " << topN;
  CHECK((scope.excludeItemIds != nullptr) + (scope.itemIds != nullptr) +
            (scope.candidates != nullptr) <= 1)
      << "a recommendation scope sets at most one of its lists";
  CHECK(!scope.screen || (!scope.excludeItemIds && !scope.itemIds && !scope.candidates))
      << "the screened route scans the whole catalogue: it takes no item or candidate list";
  const int n = static_cast<int>(topN), biases = useBiases ? 1 : 0;
  if (scope.candidates) {
    CHECK(!userIds) << "per-user candidates name their own users";
    // the known (user idx, item idx) pairs, ascending and distinct: users with their lists
    std::vector<std::pair<int64_t, int64_t>> pairs;
    size_t unknown = 0;
    for (const auto& e : *scope.candidates) {
      const size_t u = userIndex.idx(e.userId), i = itemIndex.idx(e.itemId);
      if (u == IdIndex::missingIdx || i == IdIndex::missingIdx)
        ++unknown;
      else
        pairs.emplace_back(static_cast<int64_t>(u), static_cast<int64_t>(i));
    }
    if (unknown > 0)
      LOG(WARNING) << unknown << " candidate lines name a user or item id that is not in the "
                   << "training data; skipped";
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    std::vector<int64_t> users, cptr(1, 0), cand;
    for (const auto& p : pairs) {
      if (users.empty() || users.back() != p.first) {
        users.push_back(p.first);
        cptr.push_back(cptr.back());
      }
      cand.push_back(p.second);
      ++cptr.back();
    }
    std::vector<int64_t> bptr;  // a batch's offsets, from 0
    savePairs(userIndex, itemIndex, users, fileName, topN,
              [&](const int64_t* rows, const size_t nr, int64_t* items, double* scores,
                  int32_t* counts) {
                const int64_t* p = cptr.data() + (rows - users.data());
                bptr.assign(p, p + nr + 1);
                for (auto& b : bptr) b -= p[0];
                QMFX_CHECK(qmfx_recommend_candidates(ctx, static_cast<int64_t>(nr), rows,
                                                     bptr.data(), 0, cand.data() + p[0], n,
                                                     exclude, biases, items, scores, counts));
              },
              after);
    return;
  }
  const std::vector<int64_t> users = queryRows(userIndex, userIds, "user");
  if (scope.excludeItemIds || scope.itemIds) {
    const bool deny = scope.excludeItemIds != nullptr;
    const std::vector<int64_t> list =
        sortedUnique(queryRows(itemIndex, deny ? scope.excludeItemIds : scope.itemIds, "item"));
    const int64_t nl = static_cast<int64_t>(list.size());
    savePairs(userIndex, itemIndex, users, fileName, topN,
              [&](const int64_t* rows, const size_t nr, int64_t* items, double* scores,
                  int32_t* counts) {
                const int64_t nu = static_cast<int64_t>(nr);
                if (deny)
                  QMFX_CHECK(qmfx_recommend_without(ctx, nu, rows, nl, list.data(), n, exclude,
                                                    biases, items, scores, counts));
                else
                  QMFX_CHECK(qmfx_recommend_candidates(ctx, nu, rows, nullptr, nl, list.data(), n,
                                                       exclude, biases, items, scores, counts));
              },
              after);
    return;
  }
  savePairs(userIndex, itemIndex, users, fileName, topN,
            [&](const int64_t* rows, const size_t n, int64_t* items, double* scores,
                int32_t* counts) {
              if (scope.screen)
                QMFX_CHECK(qmfx_recommend_screened(ctx, static_cast<int64_t>(n), rows,
                                                   static_cast<int>(topN), exclude,
                                                   useBiases ? 1 : 0, 0, 0, items, scores, counts));
              else
                QMFX_CHECK(qmfx_recommend(ctx, static_cast<int64_t>(n), rows,
                                          static_cast<int>(topN), exclude, useBiases ? 1 : 0,
                                          items, scores, counts));
            },
            after);
}

void Engine::saveSimilarities(qmfx_ctx* ctx, const int side, const IdIndex& index,
                              const std::string& fileName, const size_t topN, const bool cosine,
                              const std::vector<int64_t>* ids) {
  CHECK(topN >= 1 && topN <= QMFX_REC_MAX_N)
      << "the number of similar rows must be in 1.." << QMFX_REC_MAX_N << ", got " << topN;
  const std::vector<int64_t> rows = queryRows(index, ids, side == QMFX_USERS ? "user" : "item");
  savePairs(index, index, rows, fileName, topN,
            [&](const int64_t* q, const size_t n, int64_t* neighbours, double* scores,
                int32_t* counts) {
              QMFX_CHECK(qmfx_similar(ctx, side, static_cast<int64_t>(n), q,
                                      static_cast<int>(topN),
                                      cosine ? QMFX_SIM_COSINE : QMFX_SIM_DOT, 1, neighbours,
                                      scores, counts));
            });
}

void Engine::saveFactors(const FactorData& factorData, const IdIndex& index, std::ostream& out) {
  CHECK_EQ(factorData.nelems(), index.size());
  const size_t n = factorData.nelems();
  // format blocks of rows in parallel, write them in order
  const size_t block = 1 << 14;
  const size_t nblocks = (n + block - 1) / block;
  const unsigned hc = std::thread::hardware_concurrency();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(hc ? hc : 1, 32));
  for (size_t b0 = 0; b0 < nblocks; b0 += nt) {
    const size_t nb = std::min(nt, nblocks - b0);
    std::vector<std::string> parts(nb);
    ParallelExecutor::run(nb, [&](const size_t t) {
      const size_t b = (b0 + t) * block;
      formatRows(factorData, index, b, std::min(n, b + block), parts[t]);
    });
    for (const auto& p : parts) out.write(p.data(), static_cast<std::streamsize>(p.size()));
  }
}

}  // namespace qmf
