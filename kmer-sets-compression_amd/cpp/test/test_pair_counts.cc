// Host-side test of the mirror's KmerSetSetIndex::PairCounts: on one small family, the table of all nodes equals
// the sizes of the pairwise Intersection of the mirror's Get(a) and Get(b), its diagonal their Size(); a chosen,
// shuffled list of columns gives the matching sub-table.  Needs a GPU: everything runs through libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <set>
#include <string>
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
static std::uint64_t Rand() { return ksc::Mix64(0x9A1C0000 + g_ctr++); }

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
static void TestPairCounts(int n_sets, int length) {
  const auto sets = Family<K, N, KeyType>(n_sets, length);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  const KmerSetSetIndex<K, N, KeyType> index(kss);
  const int n = kss.Size();
  EXPECT_EQ(index.Nodes(), n);
  std::vector<KmerSet<K, N, KeyType>> gets;
  for (int i = 0; i < n; i++) gets.push_back(kss.Get(i, true, 4));
  std::vector<std::int64_t> want(std::size_t(n) * n);
  for (int a = 0; a < n; a++)
    for (int b = 0; b < n; b++) want[std::size_t(a) * n + b] = Intersection(gets[a], gets[b], 4).Size();
  const std::vector<std::int64_t> got = index.PairCounts();
  EXPECT_EQ(got.size(), want.size());
  EXPECT_TRUE(got == want);
  int partial = 0;
  for (int a = 0; a < n; a++) {
    EXPECT_EQ(want[std::size_t(a) * n + a], gets[a].Size());
    for (int b = 0; b < n; b++)
      if (want[std::size_t(a) * n + b] > 0 && want[std::size_t(a) * n + b] < gets[a].Size()) partial++;
  }
  EXPECT_TRUE(partial > 0);  // the expected table is not all zeros and full sets
  // chosen columns, out of order: the sub-table in the order given
  const std::vector<int> cols{n - 1, 1, 0, n / 2};
  const std::vector<std::int64_t> sub = index.PairCounts(cols);
  EXPECT_EQ(sub.size(), cols.size() * cols.size());
  if (sub.size() == cols.size() * cols.size())
    for (std::size_t a = 0; a < cols.size(); a++)
      for (std::size_t b = 0; b < cols.size(); b++)
        EXPECT_EQ(sub[a * cols.size() + b], want[std::size_t(cols[a]) * n + cols[b]]);
  std::printf("  PairCounts<%d,%d>: %d sets -> %d nodes\n", K, N, n_sets, n);
}

int main() {
  try {
    TestPairCounts<23, 14, std::uint32_t>(6, 20000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
