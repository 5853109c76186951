// Host-side test of the mirror's KmerSetSetIndex::ColorClasses: on one small family, the class table of the inputs
// equals the one counted on the host from the mirror's own Get(i) k-mers, it is ascending, its counts sum to the
// union, its sum by popcount is Spectrum and its sum over the classes with two given bits is PairCounts; a capacity
// that is too small is refused and the default policy then finds the table.  A second family of 70 sets has columns
// in both row words.  Needs a GPU: everything runs through libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "core/kmer.h"
#include "core/kmer_set.h"
#include "core/kmer_set_compact.h"
#include "core/kmer_set_set.h"
#include "core/random.h"

static int g_failed = 0, g_checks = 0;
#define EXPECT_TRUE(x)                                                        \
  do {                                                                        \
    g_checks++;                                                               \
    if (!(x)) {                                                               \
      g_failed++;                                                             \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
    }                                                                         \
  } while (0)
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))

static std::uint64_t g_ctr = 0;
static std::uint64_t Rand() { return ksc::Mix64(0xC1A55E5 + g_ctr++); }

// A correlated family: one random genome, point substitutions per member.
template <int K, int N, typename KeyType>
static std::vector<KmerSet<K, N, KeyType>> Family(int n_sets, int length) {
  std::string genome;
  for (int i = 0; i < length; i++) genome += "ACGT"[Rand() % 4];
  std::vector<KmerSet<K, N, KeyType>> out;
  for (int s = 0; s < n_sets; s++) {
    std::string g = genome;
    for (int i = 0; i < length; i++)
      if (Rand() % 300 == 0) g[i] = "ACGT"[Rand() % 4];
    std::set<std::uint64_t> kmers;
    for (int j = 0; j + K <= length; j++) kmers.insert(Kmer<K>(g.substr(j, K)).Canonical().Bits());
    out.push_back(KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end())));
  }
  return out;
}

template <int K, int N, typename KeyType>
static void TestClasses(int n_sets, int length) {
  using Index = KmerSetSetIndex<K, N, KeyType>;
  const auto sets = Family<K, N, KeyType>(n_sets, length);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  const Index index(kss);
  std::vector<int> inputs;
  for (int i = 0; i < n_sets; i++) inputs.push_back(i);

  // expected on the host: the row of every k-mer of the inputs' Get (every node is reachable from an input)
  std::map<std::uint64_t, std::uint64_t> row_of;
  for (int i = 0; i < n_sets; i++)
    for (const Kmer<K>& kmer : kss.Get(i, true, 4).Find(4)) row_of[kmer.Bits()] |= std::uint64_t(1) << i;
  std::map<std::uint64_t, std::int64_t> want;
  for (const auto& kv : row_of) want[kv.second]++;

  const std::vector<typename Index::ColorClass> got = index.ColorClasses(inputs);
  EXPECT_TRUE(want.size() > std::size_t(n_sets));
  EXPECT_EQ(got.size(), want.size());
  std::int64_t sum = 0;
  bool ascending = true, equal = got.size() == want.size();
  auto it = want.begin();
  for (std::size_t c = 0; c < got.size(); c++) {
    sum += got[c].count;
    if (c > 0) ascending = ascending && std::make_pair(got[c - 1].row[1], got[c - 1].row[0]) <
                                            std::make_pair(got[c].row[1], got[c].row[0]);
    if (equal) {
      equal = got[c].row[0] == it->first && got[c].row[1] == 0 && got[c].count == it->second;
      ++it;
    }
  }
  EXPECT_TRUE(ascending);
  EXPECT_TRUE(equal);
  EXPECT_EQ(sum, static_cast<std::int64_t>(row_of.size()));

  // the spectrum is the table's sum by popcount, the pair table its sum over the classes with both bits
  const std::vector<std::int64_t> spectrum = index.Spectrum(inputs);
  std::vector<std::int64_t> by_pop(std::size_t(n_sets) + 1, 0);
  for (const auto& cls : got) by_pop[std::size_t(__builtin_popcountll(cls.row[0]))] += cls.count;
  EXPECT_TRUE(by_pop == spectrum);
  const std::vector<std::int64_t> pairs = index.PairCounts(inputs);
  bool pairs_equal = true;
  for (int a = 0; a < n_sets; a++)
    for (int b = 0; b < n_sets; b++) {
      std::int64_t s = 0;
      for (const auto& cls : got)
        if (((cls.row[0] >> a) & 1) && ((cls.row[0] >> b) & 1)) s += cls.count;
      pairs_equal = pairs_equal && s == pairs[std::size_t(a) * std::size_t(n_sets) + std::size_t(b)];
    }
  EXPECT_TRUE(pairs_equal);

  // all nodes as columns: the same k-mers; exactly enough room is enough, one class less is refused
  const std::vector<typename Index::ColorClass> every = index.ColorClasses();
  std::int64_t sum_every = 0;
  for (const auto& cls : every) sum_every += cls.count;
  EXPECT_EQ(sum_every, sum);
  EXPECT_EQ(index.ColorClasses(inputs, static_cast<std::int64_t>(want.size())).size(), want.size());
  bool refused = false;
  try {
    index.ColorClasses(inputs, static_cast<std::int64_t>(want.size()) - 1);
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("capacity") != std::string::npos;
  }
  EXPECT_TRUE(refused);
  EXPECT_EQ(index.ColorClasses(inputs).size(), want.size());  // the index still serves
  std::printf("  ColorClasses<%d,%d>: %d sets -> %d nodes, %zu classes of %lld k-mers\n", K, N, n_sets, kss.Size(),
              want.size(), static_cast<long long>(sum));
}

// More than 64 columns: the mirror unpacks rows[2c + 1] into row[1].  The structure is built with a few iterations
// only, so that it has the inputs and a handful of internal nodes.
template <int K, int N, typename KeyType>
static void TestWideClasses(int n_sets, int length) {
  using Index = KmerSetSetIndex<K, N, KeyType>;
  using Row = std::pair<std::uint64_t, std::uint64_t>;  // (row[1], row[0]): ordered as the call orders
  const auto sets = Family<K, N, KeyType>(n_sets, length);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4, ksc::SampleBucketIds(N, ksc::BucketSeedFromEnv()), 4);
  const Index index(kss);
  std::vector<int> inputs;
  for (int i = 0; i < n_sets; i++) inputs.push_back(i);

  std::map<std::uint64_t, Row> row_of;
  for (int i = 0; i < n_sets; i++)
    for (const Kmer<K>& kmer : kss.Get(i, true, 4).Find(4)) {
      Row& r = row_of[kmer.Bits()];
      (i < 64 ? r.second : r.first) |= std::uint64_t(1) << (i & 63);
    }
  std::map<Row, std::int64_t> want;
  for (const auto& kv : row_of) want[kv.second]++;

  const std::vector<typename Index::ColorClass> got = index.ColorClasses(inputs);
  EXPECT_EQ(got.size(), want.size());
  bool equal = got.size() == want.size(), second_word = false;
  std::int64_t sum = 0;
  std::vector<std::int64_t> by_pop(std::size_t(n_sets) + 1, 0);
  auto it = want.begin();
  for (std::size_t c = 0; c < got.size() && equal; c++, ++it) {
    equal = got[c].row[1] == it->first.first && got[c].row[0] == it->first.second && got[c].count == it->second;
    second_word = second_word || got[c].row[1] != 0;
    sum += got[c].count;
    by_pop[std::size_t(__builtin_popcountll(got[c].row[0]) + __builtin_popcountll(got[c].row[1]))] += got[c].count;
  }
  EXPECT_TRUE(equal);
  EXPECT_TRUE(second_word);
  EXPECT_EQ(sum, static_cast<std::int64_t>(row_of.size()));
  EXPECT_TRUE(by_pop == index.Spectrum(inputs));
  // the class of the k-mers that every set holds: all of word 0 and the low n_sets - 64 bits of word 1
  const Row core{(std::uint64_t(1) << (n_sets - 64)) - 1, ~std::uint64_t(0)};
  EXPECT_TRUE(want.count(core) == 1);
  EXPECT_TRUE(!got.empty() && got.back().row[1] == core.first && got.back().row[0] == core.second);
  std::printf("  ColorClasses<%d,%d>: %d sets -> %d nodes, %zu classes of %lld k-mers, both row words\n", K, N, n_sets,
              kss.Size(), want.size(), static_cast<long long>(sum));
}

int main() {
  try {
    TestClasses<23, 14, std::uint32_t>(6, 20000);
    TestWideClasses<23, 14, std::uint32_t>(70, 20000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
